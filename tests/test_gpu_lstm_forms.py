"""Every LSTM recurrence form behind mts_lstm_fwd / mts_lstm_bwd (generic fp32 / bf16, CU-quad bf16 and fp32, CU-pair bf16, persistent MFMA bf16)
against the fp64 reference of tests/lstm_oracle.py, on the case table and under the bounds kept there: out, dxproj and dW_hh, exact zeros on the
rows past a document's end, the saved gates and cells, the backward in two calls, one launch-to-launch repeat per form, and the contract corners
(ndir = 1, lengths = NULL, b_hh = NULL, a document of length 0, a length above L).

Which kernels ran is proved by the saved state: the bf16 CU-quad recurrences keep step-major blocks, the other forms the row-major layout of
mts.h, and each case reads the state through the layout of the form it expects (lstm_oracle.saved_state_index).  The persistent MFMA form is reached
the way INTEGRATION.md tells users to reach it, MTS_LSTM_PAIR=0 in the environment; the library reads that once per host thread, so those cases run
on a fresh thread started with the variable set."""
import os
import threading

import pytest
import torch

from tests import lstm_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _launch(case, ops):
    """forward + backward of one case on the calling thread -> dict of device tensors (every output pre-filled with NaN)"""
    H, B, Lq, nd, dt = case.H, case.B, case.L, case.ndir, case.dtype
    N = B * Lq
    inp = O.inputs(case)
    xd, dd, wd = inp['xproj'].to(dt).to(DEV), inp['dout'].to(dt).to(DEV), inp['w_hh'].to(DEV)
    bd = inp['b_hh'].to(DEV) if case.bias else None
    li = None if case.lengths is None else torch.tensor(case.lengths, dtype=torch.int32, device=DEV)
    nan = lambda *s, dtype: torch.full(s, float('nan'), dtype=dtype, device=DEV)
    r = dict(out=nan(N, nd * H, dtype=dt), gates=nan(N, nd * 4 * H, dtype=dt), cells=nan(N, nd * H, dtype=torch.float32),
             dxproj=nan(N, nd * 4 * H, dtype=dt), dw_hh=nan(nd, 4 * H, H, dtype=torch.float32))
    ops.lstm_fwd(xd, wd, bd, li, B, Lq, H, nd, r['out'], r['gates'], r['cells'])
    if case.refused_bwd:
        ws = ops.lstm_workspace(dt, B, Lq, H, nd, DEV, tag='test_forms')
        for call in (lambda: ops.lstm_bwd(wd, li, r['out'], r['gates'], r['cells'], dd, B, Lq, H, nd, r['dxproj'], r['dw_hh']),
                     lambda: ops.lstm_bwd_whh(li, r['out'], r['dxproj'], B, Lq, H, nd, r['dw_hh'], ws)):
            with pytest.raises(NotImplementedError, match='must be a multiple of'):
                call()
        torch.cuda.synchronize()
        return r
    ops.lstm_bwd(wd, li, r['out'], r['gates'], r['cells'], dd, B, Lq, H, nd, r['dxproj'], r['dw_hh'])
    if case.two_call:
        r['dxproj2'], r['dw_hh2'] = nan(N, nd * 4 * H, dtype=dt), nan(nd, 4 * H, H, dtype=torch.float32)
        ws = ops.lstm_workspace(dt, B, Lq, H, nd, DEV, tag='test_forms')
        ops.lstm_bwd_recurrence(wd, li, r['out'], r['gates'], r['cells'], dd, B, Lq, H, nd, r['dxproj2'], ws)
        ev = torch.cuda.Event()
        ev.record()
        side = torch.cuda.Stream()
        side.wait_event(ev)
        with torch.cuda.stream(side):
            ops.lstm_bwd_whh(li, r['out'], r['dxproj2'], B, Lq, H, nd, r['dw_hh2'], ws)
    torch.cuda.synchronize()
    return r


def _run(case):
    """-> (first run, second run or None), under the options / environment that select the case's form"""
    from multimodaltopicsegmentation_amd import _lib as L, ops
    res = {}

    def body():
        try:
            if case.lstm_parts != 4:
                L.check(L.lib.mts_set_option(b'lstm_parts', case.lstm_parts))
            try:
                res['a'] = _launch(case, ops)
                res['b'] = _launch(case, ops) if case.repeat else None
                L.check_async()
            finally:
                L.check(L.lib.mts_set_option(b'lstm_parts', 4))
        except BaseException as e:          # noqa: BLE001 -- handed to the test's own thread
            res['error'] = e

    if case.pair_env:
        body()
    else:
        old = os.environ.get('MTS_LSTM_PAIR')
        os.environ['MTS_LSTM_PAIR'] = '0'
        try:
            th = threading.Thread(target=body)
            th.start()
            th.join()
        finally:
            if old is None:
                del os.environ['MTS_LSTM_PAIR']
            else:
                os.environ['MTS_LSTM_PAIR'] = old
    if 'error' in res:
        raise res['error']
    return res['a'], res['b']


@pytest.mark.parametrize('case', O.CASES, ids=lambda c: c.id)
def test_form_against_fp64(case):
    got, again = _run(case)
    rows = O.valid_rows(case)
    if case.refused_bwd:
        # nothing was launched by the refused calls: the gradient buffers still hold their fill; the forward is the generic kernel's
        assert bool(torch.isnan(got['dxproj'].float()).all()) and bool(torch.isnan(got['dw_hh']).all())
        o = got['out'].float().cpu()
        g, c = O.canonical_state(case, got['gates'].float().cpu(), got['cells'].cpu())
        assert float(o[~rows].abs().max()) == 0.0
        assert O.excess(case, 'out', o) <= 1.0 and O.excess(case, 'gates', g, rows=rows) <= 1.0 and O.excess(case, 'cells', c, rows=rows) <= 1.0
        return
    cpu = {k: v.float().cpu() for k, v in got.items()}
    cpu['gates'], cpu['cells'] = O.canonical_state(case, cpu['gates'], cpu['cells'])
    figures = {q: O.excess(case, q, cpu[q], rows=rows if q in ('gates', 'cells') else None) for q in O.QUANTITIES}
    print(case.id, case.form, {q: round(v, 3) for q, v in figures.items()})
    if (~rows).any():       # rows at and past a document's length: exact zeros, both directions
        assert float(cpu['out'][~rows].abs().max()) == 0.0, 'out past a document end'
        assert float(cpu['dxproj'][~rows].abs().max()) == 0.0, 'dxproj past a document end'
    # the saved state first: it says which kernels ran
    assert figures['gates'] <= 1.0 and figures['cells'] <= 1.0, (case.form, figures)
    assert figures['out'] <= 1.0 and figures['dxproj'] <= 1.0 and figures['dw_hh'] <= 1.0, figures
    if case.two_call:
        assert torch.equal(_bits(got['dxproj']), _bits(got['dxproj2'])), 'two-call dxproj differs from the single call'
        assert torch.equal(_bits(got['dw_hh']), _bits(got['dw_hh2'])), 'two-call dW_hh differs from the single call'
        assert O.excess(case, 'dxproj', cpu['dxproj2']) <= 1.0 and O.excess(case, 'dw_hh', cpu['dw_hh2']) <= 1.0
    if case.repeat:
        for q in ('out', 'dxproj', 'dw_hh'):
            assert torch.equal(_bits(got[q]), _bits(again[q])), f'{q} differs from launch to launch'
