"""CPU pins of tests/lstm_oracle.py, the reference, restatement, case table and bounds that tests/test_gpu_lstm_forms.py holds the LSTM recurrence
kernels to: the two statements of the reference against each other and against torch's own nn.LSTM, the measured table T against a fresh
measurement, the mutant-free restatement inside every bound and every planted error outside one, the dispatch restated, and the coverage of the
case table."""
import pytest
import torch

from oracle import restatement as R
from tests import lstm_oracle as O

RUN = [c for c in O.CASES if not c.refused_bwd]


def test_dispatch_restated():
    bf, fp = torch.bfloat16, torch.float32
    assert O.expected_form(bf, 256) == 'quad_bf16' and O.expected_form(fp, 256) == 'quad_fp32'
    assert O.expected_form(bf, 256, lstm_parts=2) == 'pair_bf16' and O.expected_form(fp, 256, lstm_parts=2) == 'generic'
    assert O.expected_form(bf, 256, pair_env=False) == 'mfma_bf16' and O.expected_form(bf, 256, 2, False) == 'mfma_bf16'
    assert O.expected_form(fp, 256, pair_env=False) == 'generic'
    for H in (24, 25, 64, 104, 255, 257, 1024):
        for dt in (bf, fp):
            for parts in (2, 4):
                for env in (True, False):
                    assert O.expected_form(dt, H, parts, env) == 'generic'


def test_cases_cover_every_form():
    assert len({c.id for c in O.CASES}) == len(O.CASES)
    by_form = {f: [c for c in RUN if c.form == f] for f in O.FORMS}
    assert all(by_form[f] for f in O.FORMS), {f: len(v) for f, v in by_form.items()}
    assert {c.dtype for c in by_form['generic']} == {torch.float32, torch.bfloat16}
    for f, cases in by_form.items():
        assert any(not c.two_call for c in cases), f                                  # the single call runs on every case; some run nothing else
        assert any(c.two_call for c in cases), f
        assert any(c.repeat for c in cases), f
        assert any(c.ndir == 1 for c in cases), f
        assert any(c.lengths is None for c in cases), f
        assert any(not c.bias for c in cases), f
        assert any(c.lengths is not None and 0 in c.lengths and max(c.lengths) > c.L for c in cases), f
        if f != 'generic':
            assert all(c.H == 256 for c in cases)
            # two groups of 16 with a single document in the last, group maxima odd and even; a partly filled single group, even step count
            big = [c for c in cases if c.B == 17]
            assert big and all(max(c.lengths[:16]) % 2 == 1 and c.lengths[16] % 2 == 0 and {1, 2, 8, 9} <= set(c.lengths) for c in big)
            assert any(c.B == 3 and c.lengths == (8, 7, 2) for c in cases)
    gen = by_form['generic']
    assert {c.H for c in gen} >= {24, 28, 104, 256, 1024}
    for H in (24, 104):
        for dt in (torch.float32, torch.bfloat16):
            assert {c.B for c in gen if c.H == H and c.dtype == dt} >= {1, 9}, (H, dt)
    assert {c.B for c in gen if c.H == 28 and c.dtype == torch.float32} >= {1, 9}
    assert any(c.H == 1024 and c.dtype == torch.float32 and (c.B, c.L) == (9, 3) for c in gen)
    assert any(c.H == 256 and c.dtype == torch.float32 and c.lstm_parts == 2 for c in gen)
    # H = 25: the forward in both dtypes (fp32 with one document and with a last group of one); the backward is refused in both
    refused = [c for c in O.CASES if c.refused_bwd]
    assert {(c.dtype, c.B) for c in refused} >= {(torch.float32, 1), (torch.float32, 9), (torch.bfloat16, 9)}
    assert all(c.H == 25 and c.form == 'generic' for c in refused)
    assert all(c.H % (8 if c.dtype == torch.bfloat16 else 4) == 0 for c in RUN)
    assert all(c.B * c.L <= 200 for c in O.CASES)
    # no negative length is ever fed to a kernel: that corner is closed by reading the clamps
    assert all(min(c.lengths) >= 0 for c in O.CASES if c.lengths is not None)


@pytest.mark.parametrize('case', O.CASES, ids=lambda c: c.id)
def test_batched_and_per_document_references_agree(case):
    ref = O.reference(case)
    assert float((ref['out'] - ref['out_batched']).abs().max()) <= 1e-13
    rows = O.valid_rows(case)
    assert float(ref['out'][~rows].abs().max()) == 0.0 if (~rows).any() else True
    assert float(ref['dxproj'][~rows].abs().max()) == 0.0 if (~rows).any() else True
    # h = o * tanh(c) ties the saved state to `out`
    H, nd = case.H, case.ndir
    g, c = ref['gates'].view(-1, nd, 4, H), ref['cells'].view(-1, nd, H)
    assert float((g[:, :, 3] * torch.tanh(c) - ref['out'].view(-1, nd, H)).abs().max()) <= 1e-13


def test_reference_against_torch_lstm():
    case = O.BY_ID['generic-fp32-H24-B9L7']
    inp, ref = O.inputs(case), O.reference(case)
    H, B, L = case.H, case.B, case.L
    lstm = torch.nn.LSTM(4 * H, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for d, sfx in enumerate(('', '_reverse')):
            getattr(lstm, 'weight_ih_l0' + sfx).copy_(torch.eye(4 * H))
            getattr(lstm, 'weight_hh_l0' + sfx).copy_(inp['w_hh'][d])
            getattr(lstm, 'bias_ih_l0' + sfx).zero_()
            getattr(lstm, 'bias_hh_l0' + sfx).copy_(inp['b_hh'][d])
    xp = inp['xproj'].double().view(B, L, 2, 4 * H)
    lens = torch.tensor(case.eff_lengths)
    outs = []
    for d in range(2):          # nn.LSTM feeds both directions the same input: run it once per direction's own projection
        packed = torch.nn.utils.rnn.pack_padded_sequence(xp[:, :, d], lens, batch_first=True, enforce_sorted=False)
        y, _ = torch.nn.utils.rnn.pad_packed_sequence(lstm(packed)[0], batch_first=True, total_length=L)
        outs.append(y[:, :, d * H:(d + 1) * H])
    want = torch.cat(outs, 2).reshape(B * L, 2 * H).detach()
    assert float((ref['out'] - want).abs().max()) <= 1e-12
    assert float((ref['out'] - torch.cat([R.lstm_direction_batched(xp[:, :, d], lens, torch.eye(4 * H, dtype=torch.float64), inp['w_hh'][d].double(),
                                                                   torch.zeros(4 * H, dtype=torch.float64), inp['b_hh'][d].double(), d == 1)
                                          for d in range(2)], 2).reshape(B * L, 2 * H)).abs().max()) <= 1e-12


def test_state_index_is_one_to_one():
    for case in RUN:
        gi, ci = O.saved_state_index(case)
        rows = O.valid_rows(case)
        for idx, width in ((gi, 4 * case.H), (ci, case.H)):
            assert bool((idx[~rows] == -1).all()) and bool((idx[rows] >= 0).all())
            flat = idx[rows].reshape(-1)
            assert flat.numel() == flat.unique().numel() and int(flat.max()) < case.B * case.L * case.ndir * width, case.id
    # the step-major blocks differ from the row-major layout exactly on the bf16 CU-quad form
    a, b = O.BY_ID['quad_bf16-B17L9'], O.BY_ID['mfma_bf16-B17L9']
    assert not torch.equal(O.saved_state_index(a)[0], O.saved_state_index(b)[0])
    assert torch.equal(O.saved_state_index(O.BY_ID['pair_bf16-B17L9'])[1], O.saved_state_index(b)[1])


def test_measured_table_is_current():
    """T holds the measured error of the mutant-free restatement: never above the table, and the table is no looser than 5 % over it"""
    bf = [c for c in O.CASES if c.dtype == torch.bfloat16]          # the refused backward's case too: its forward is compared
    assert set(O.T) == {c.id for c in bf}
    for c in bf:
        t = O.measure_t(c)
        for q in O.QUANTITIES:
            assert 0.95 * O.T[c.id][q] <= t[q] <= O.T[c.id][q], (c.id, q, t[q], O.T[c.id][q])
    assert O.M == 4.0 and not O.RAISED


@pytest.mark.parametrize('case', RUN, ids=lambda c: c.id)
def test_restatement_is_inside_every_bound(case):
    got = O.restatement(case)
    for q in O.QUANTITIES:
        e = O.excess(case, q, got[q])
        # bf16: 1 / M by construction of T (less where the bf16 storage term helps); fp32: fp64 arithmetic stored in fp32 is far inside
        assert e <= (1 / O.M + 1e-9 if case.dtype == torch.bfloat16 else 0.05), (q, e)
    rows = O.valid_rows(case)
    if (~rows).any():
        assert float(got['out'][~rows].abs().max()) == 0.0 and float(got['dxproj'][~rows].abs().max()) == 0.0


@pytest.mark.parametrize('form', O.FORMS)
@pytest.mark.parametrize('mutant', O.MUTANTS)
def test_every_mutant_is_outside_a_bound(mutant, form):
    """on at least one case of every form (for the generic form: in each dtype) the planted error breaks a bound that the GPU test applies"""
    for dt in ({c.dtype for c in RUN if c.form == form}):
        cases = [c for c in RUN if c.form == form and c.dtype == dt and O.applies(mutant, c)]
        assert cases, (mutant, form, dt)
        worst = 0.0
        for c in cases:
            got = O.restatement(c, mutant=mutant)
            worst = max(worst, max(O.excess(c, q, got[q]) for q in O.QUANTITIES))     # the GPU test compares all five on every form
            if worst > 1.0:
                break
        assert worst > 1.0, (mutant, form, dt, worst)


def test_padded_rows_mutant_breaks_the_exact_zero_check():
    case = O.BY_ID['pair_bf16-B3L8']
    got = O.restatement(case, mutant='padded_dxproj')
    assert float(got['dxproj'][~O.valid_rows(case)].abs().max()) > 0.0
