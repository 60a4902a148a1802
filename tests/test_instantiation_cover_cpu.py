"""The written-down list of what "every instantiation" means for the three host-side dispatchers that pick a kernel template from the
shape: RMSNorm (csrc/rmsnorm.hip), the domain-switched heads' parameter pass (csrc/switch_head.hip) and full self-attention
(csrc/full_attn.hip).  Each selection rule is restated here in Python next to the source line it restates, and the case lists of the
GPU tests are checked against it: their union has to reach every instantiation the rule can select.  Needs no GPU: the case lists are
plain module-level data.  Whoever adds an NV, a KK or a chunk adds a case."""
from tests.test_gpu_full_attention import CASES as FULL_CASES, MODES as FULL_MODES, _case as full_case, _refused_in as full_refused_in
from tests.test_gpu_recurrent_longt5 import RMS_CASES
from tests.test_gpu_switch import KERNEL_CASES as SWITCH_CASES


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ RMSNorm
def rms_nv(D):
    """static int rms_nv(int D) { const int nv = (D + 255) / 256; return nv <= 1 ? 1 : nv <= 2 ? 2 : nv <= 4 ? 4 : nv <= 8 ? 8 : 0; }
    behind rms_check's  MTS_UNSUPPORTED(D % 4 == 0 && D <= 2048, ...)"""
    if D % 4 or D > 2048:
        return 0
    nv = (D + 255) // 256
    return 1 if nv <= 1 else 2 if nv <= 2 else 4 if nv <= 4 else 8


def rms_last_slot(D):
    """columns of slot NV - 1 (lane l holds columns 4 l + 256 k, k < NV, where c < D): 256 = fully live, 1..255 = partially, 0 = masked"""
    return max(0, min(256, D - 256 * (rms_nv(D) - 1)))


def rms_required():
    need = set()
    for D in range(4, 2049, 4):                        # everything rms_check admits
        live = rms_last_slot(D)
        if live:
            need.add((rms_nv(D), 'full' if live == 256 else 'partial'))
    need.add('D % 16 != 0')                            # rms_dw_reduce_kernel: grid ceil(D / 16), the last workgroup partly idle
    need.add('backward strides, rows % 4 != 0')        # RMS_BWD_BLOCKS = 256 workgroups x RMS_WAVES = 4 rows: rows > 1024
    return need


def rms_reached(cases):
    got = set()
    for rows, D in cases:
        assert rms_nv(D), (rows, D)
        live = rms_last_slot(D)
        if live:
            got.add((rms_nv(D), 'full' if live == 256 else 'partial'))
        if D % 16:
            got.add('D % 16 != 0')
        if ceil_div(rows, 4) > 256 and rows % 4:
            got.add('backward strides, rows % 4 != 0')
    return got


# ------------------------------------------------------------------------------------------------ switched heads, parameter pass
SW_WAVES, SW_MAX_BLOCKS = 4, 512                       # #define SW_WAVES 4, #define SW_MAX_BLOCKS 512


def sw_pick_nv(D):
    """static inline int sw_pick_nv(int D) { const int need = ceil_div(D, 256); if (need <= 1) return 1; if (need <= 2) return 2;
    if (need <= 4) return 4; if (need <= 16) return 8; return 0; }"""
    need = ceil_div(D, 256)
    return 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8 if need <= 16 else 0


def sw_instantiation(D):
    """(NV, FULL, chunks) or None = refused:  const int chunks = ceil_div(D, nv * 256);  and in sw_params_launch
    if (D == NV * 256) switch_head_bwd_params_kernel<T, NV, true> else <T, NV, false>"""
    nv = sw_pick_nv(D)
    if D % 4 or not nv:                                # sw_check: D % 4 == 0;  MTS_UNSUPPORTED(nv > 0, "... D=%d must be <= 4096")
        return None
    return nv, D == nv * 256, ceil_div(D, nv * 256)


def sw_required():
    need = {sw_instantiation(D) for D in range(4, 4097, 4)}
    assert need == {(1, False, 1), (1, True, 1), (2, False, 1), (2, True, 1), (4, False, 1), (4, True, 1), (8, False, 1), (8, True, 1),
                    (8, False, 2)}
    assert sw_instantiation(4100) is None
    need |= {f'n_out = {n}' for n in (1, 2, 3, 4)}     # sw_check: n_out >= 1 && n_out <= 4
    need.add('pass strides, rows % 4 != 0')            # blocks = min(SW_MAX_BLOCKS, ceil_div(B * L, SW_WAVES))
    return need


def sw_reached(cases):
    got = set()
    for B, L, D, n_out, doms in cases:
        assert sw_instantiation(D) is not None and len(doms) == B, (B, L, D)
        got.add(sw_instantiation(D))
        got.add(f'n_out = {n_out}')
        if ceil_div(B * L, SW_WAVES) > SW_MAX_BLOCKS and (B * L) % SW_WAVES:
            got.add('pass strides, rows % 4 != 0')
    return got


# ------------------------------------------------------------------------------------------------ full self-attention
def attn_row_stride(hd, esize):
    """int bytes = ((hd * esize + 15) / 16) * 16; if (((bytes / 16) & 1) == 0) bytes += 16; return bytes;   (attn_tile.h)"""
    b = (hd * esize + 15) // 16 * 16
    return b + 16 if (b // 16) % 2 == 0 else b


def full_generic_lds(hd, esize):
    """return (size_t)4 * FT * rs + (size_t)(2 * FT * PS + 2 * FT) * sizeof(float);   with FT = 32, PS = 33: 128 rs + 8704"""
    return 4 * 32 * attn_row_stride(hd, esize) + (2 * 32 * 33 + 2 * 32) * 4


def full_path(hd, mode):
    """'refused', ('mfma', KK) or ('generic', MAXU) for a head dim in one of the test's modes (mfma: bf16; generic: bf16 with option
    full_mfma 0; fp32).  full_fill:
      MTS_UNSUPPORTED(hd % vec == 0 && hd <= 512, ...)  with vec = dtype == MTS_F32 ? 4 : 8
      MTS_UNSUPPORTED(full_generic_lds(a.rs) <= 160 * 1024, ...)
    full_use_mfma:  dtype == MTS_BF16 && g_full_mfma && a.hd % 32 == 0 && a.hd <= 256   ->  FULL_KK_SWITCH(a.hd / 32, ...), KK = 1 .. 8
    full_fwd_launch / full_bwd_launch:  a.hd > 256 ? full_*_kernel<T, 16> : full_*_kernel<T, 8>"""
    esize, vec = (4, 4) if mode == 'fp32' else (2, 8)
    if hd % vec or hd > 512 or full_generic_lds(hd, esize) > 160 * 1024:
        return 'refused'
    if mode == 'mfma' and hd % 32 == 0 and hd <= 256:
        return 'mfma', hd // 32
    return 'generic', 16 if hd > 256 else 8


def full_required():
    need = {(mode, full_path(hd, mode)) for mode in FULL_MODES for hd in range(4, 513, 4) if full_path(hd, mode) != 'refused'}
    assert need == ({('mfma', ('mfma', kk)) for kk in range(1, 9)} | {(m, ('generic', u)) for m in FULL_MODES for u in (8, 16)})
    need.discard(('mfma', ('generic', 8)))             # the same launch as ('generic', ('generic', 8)): the option only matters where
    need.discard(('mfma', ('generic', 16)))            # the matrix-core kernels apply
    return need | {'refused in bf16', 'refused in fp32'}


def full_reached(cases):
    got = set()
    for name in cases:
        assert cases[name] is FULL_CASES[name]
        B, Lq, D, heads = full_case(name)[:4]
        declared = full_refused_in(name)
        for mode in FULL_MODES:
            path = full_path(D // heads, mode)
            assert (path == 'refused') == (mode in declared), (name, mode, path, declared)      # the case says what the rule says
            got.add(('refused in fp32' if mode == 'fp32' else 'refused in bf16') if path == 'refused' else (mode, path))
    return got


# ------------------------------------------------------------------------------------------------ the tests
def _missing(need, got):
    return sorted(map(str, need - got))


def test_rmsnorm_cases_reach_every_instantiation():
    assert rms_nv(2052) == 0 and rms_nv(6) == 0        # the two refusals of the "refuses ... before launch" test
    assert not _missing(rms_required(), rms_reached(RMS_CASES)), _missing(rms_required(), rms_reached(RMS_CASES))


def test_switch_cases_reach_every_instantiation():
    assert not _missing(sw_required(), sw_reached(SWITCH_CASES)), _missing(sw_required(), sw_reached(SWITCH_CASES))


def test_full_attention_cases_reach_every_instantiation():
    # the LDS bound of test_the_lds_bound_is_where_full_fill_puts_it, from the formula
    assert full_generic_lds(300, 4) == 162304 and full_generic_lds(304, 4) == 166400 and full_generic_lds(512, 2) == 141824
    assert full_path(300, 'fp32') == ('generic', 16) and full_path(304, 'fp32') == 'refused' and full_path(512, 'generic') == ('generic', 16)
    assert full_path(264, 'mfma') == ('generic', 16)   # 264 % 32 != 0
    assert not _missing(full_required(), full_reached(FULL_CASES)), _missing(full_required(), full_reached(FULL_CASES))


def test_the_lists_before_this_cover_was_written_down_miss_what_it_says():
    """not vacuous: the case lists as they stood before the cases of this file's concern were appended (the lists are append-only: a
    case's position seeds it) miss whole instantiations"""
    assert _missing(rms_required(), rms_reached(RMS_CASES[:4])) == sorted(map(str, [
        (1, 'full'), (2, 'partial'), (4, 'full'), (4, 'partial'), (8, 'full'), (8, 'partial'), 'D % 16 != 0',
        'backward strides, rows % 4 != 0']))
    assert _missing(sw_required(), sw_reached(SWITCH_CASES[:7])) == sorted(map(str, [
        (1, True, 1), (2, False, 1), (4, True, 1), (8, False, 1), (8, True, 1), (8, False, 2), 'n_out = 3', 'n_out = 4',
        'pass strides, rows % 4 != 0']))
    old = {n: FULL_CASES[n] for n in list(FULL_CASES)[:11]}
    assert _missing(full_required(), full_reached(old)) == sorted(map(str, [
        ('mfma', ('mfma', 3)), ('mfma', ('mfma', 4)), ('mfma', ('mfma', 5)), ('mfma', ('mfma', 6)), ('generic', ('generic', 16)),
        ('fp32', ('generic', 16)), 'refused in bf16', 'refused in fp32']))
