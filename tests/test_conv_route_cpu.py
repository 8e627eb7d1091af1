"""sparse._conv_route: which sparse-convolution kernel a launch takes, as a table.  No library, no tensors: the two planners are
stubs and the rulebook is a stand-in with ``coords`` / ``K`` only.  The expected values were written down from the four branches of
the launch function this table replaced, not produced by the code under test."""
import os
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP, BF, X3 = 0, 1, 2                       # precision.FMT_FP32 / FMT_BF16 / FMT_X3
N = 40_000                                 # _RS_MIN_ROWS of the table
SUBM, DOWN = SimpleNamespace(coords=object(), K=27), SimpleNamespace(coords=None, K=8)
TS_PLAN = (128, 192)
PAIRS, PAIRS_ROWS = (32, 1, False), (64, 2, True)        # what the stub planner answers for u3d_spconv_plan / u3d_spconv_plan_bf16a

# (toggles on, globals patched, (Cs, Cd, n_dst, rulebook, format, shadow present, statistics wanted)) -> (route, format, plan)
CASES = [
    # every toggle off: the pair-list kernel of the format; fp32 wherever the source channels are no multiple of 32
    ('', {}, (32, 32, N, SUBM, FP, False, False), ('pairs', FP, PAIRS)),
    ('', {}, (32, 32, N, SUBM, X3, False, True), ('pairs', X3, PAIRS)),
    ('', {}, (96, 48, N, DOWN, X3, False, False), ('pairs', X3, PAIRS)),
    ('', {}, (32, 32, N, SUBM, BF, False, False), ('pairs', BF, PAIRS)),
    ('', {}, (32, 32, N, SUBM, BF, True, False), ('pairs', BF, PAIRS_ROWS)),
    ('', {}, (96, 32, 5, DOWN, BF, True, True), ('pairs', BF, PAIRS_ROWS)),
    ('', {}, (16, 32, N, SUBM, X3, False, False), ('pairs', FP, PAIRS)),
    ('', {}, (16, 32, N, SUBM, BF, True, False), ('pairs', FP, PAIRS)),
    ('', {'_EPILOGUE_STATS': True}, (32, 32, N, SUBM, X3, False, True), ('pairs', X3, PAIRS)),
    # register-stationary, three planes
    ('rs', {}, (32, 32, N, SUBM, X3, False, False), ('rs', X3, 320)),
    ('rs', {}, (96, 32, N, SUBM, X3, False, False), ('rs', X3, 320)),
    ('rs', {}, (32, 32, N - 1, SUBM, X3, False, False), ('pairs', X3, PAIRS)),
    ('rs', {}, (32, 48, N, SUBM, X3, False, False), ('pairs', X3, PAIRS)),
    ('rs', {}, (16, 32, N, SUBM, X3, False, False), ('pairs', FP, PAIRS)),
    ('rs', {}, (32, 32, N, DOWN, X3, False, False), ('pairs', X3, PAIRS)),
    ('rs', {}, (32, 32, N, SUBM, FP, False, False), ('pairs', FP, PAIRS)),
    ('rs', {}, (32, 32, N, SUBM, BF, True, False), ('pairs', BF, PAIRS_ROWS)),
    ('rs', {'_RS_MAX_BLOCKS': 3}, (96, 32, N, SUBM, X3, False, False), ('rs', X3, 320)),
    ('rs', {'_RS_MAX_BLOCKS': 2}, (96, 32, N, SUBM, X3, False, False), ('pairs', X3, PAIRS)),
    ('rs', {}, (32, 32, N, SUBM, X3, False, True), ('rs', X3, 320)),                    # statistics asked for, but not from the epilogue
    ('rs', {'_EPILOGUE_STATS': True}, (32, 32, N, SUBM, X3, False, False), ('rs', X3, 320)),
    ('rs', {'_EPILOGUE_STATS': True}, (32, 32, N, SUBM, X3, False, True), ('pairs', X3, PAIRS)),
    # register-stationary, bf16 rows: needs the shadow, ignores the statistics request
    ('rsb', {}, (32, 32, N, SUBM, BF, True, False), ('rsb', BF, 448)),
    ('rsb', {'_EPILOGUE_STATS': True}, (96, 32, N, SUBM, BF, True, True), ('rsb', BF, 448)),
    ('rsb', {}, (32, 32, N, SUBM, BF, False, False), ('pairs', BF, PAIRS)),
    ('rsb', {}, (32, 32, N, SUBM, X3, False, False), ('pairs', X3, PAIRS)),
    ('rsb', {}, (32, 32, N, SUBM, FP, False, False), ('pairs', FP, PAIRS)),
    ('rsb', {}, (32, 32, N - 1, SUBM, BF, True, False), ('pairs', BF, PAIRS_ROWS)),
    ('rsb', {}, (32, 48, N, SUBM, BF, True, False), ('pairs', BF, PAIRS_ROWS)),
    ('rsb', {}, (16, 32, N, SUBM, BF, True, False), ('pairs', FP, PAIRS)),
    ('rsb', {}, (32, 32, N, DOWN, BF, True, False), ('pairs', BF, PAIRS_ROWS)),
    ('rsb', {'_RS_MAX_BLOCKS': 3}, (96, 32, N, SUBM, BF, True, False), ('rsb', BF, 448)),
    ('rsb', {'_RS_MAX_BLOCKS': 2}, (96, 32, N, SUBM, BF, True, False), ('pairs', BF, PAIRS_ROWS)),
    # tile-stationary: the planner decides the shapes (no row minimum, no block limit, no test of Cd here)
    ('ts', {}, (32, 32, N, SUBM, X3, False, False), ('ts', X3, TS_PLAN)),
    ('ts', {}, (96, 48, 5, SUBM, X3, False, False), ('ts', X3, TS_PLAN)),
    ('ts', {'_RS_MAX_BLOCKS': 0}, (32, 32, N, SUBM, X3, False, False), ('ts', X3, TS_PLAN)),
    ('ts', {'_ts_plan': None}, (32, 32, N, SUBM, X3, False, False), ('pairs', X3, PAIRS)),
    ('ts', {}, (16, 32, N, SUBM, X3, False, False), ('pairs', FP, PAIRS)),
    ('ts', {}, (32, 32, N, DOWN, X3, False, False), ('pairs', X3, PAIRS)),
    ('ts', {}, (32, 32, N, SUBM, FP, False, False), ('pairs', FP, PAIRS)),
    ('ts', {}, (32, 32, N, SUBM, BF, True, False), ('pairs', BF, PAIRS_ROWS)),
    ('ts', {}, (32, 32, N, SUBM, X3, False, True), ('ts', X3, TS_PLAN)),
    ('ts', {'_EPILOGUE_STATS': True}, (32, 32, N, SUBM, X3, False, True), ('pairs', X3, PAIRS)),
    # all three on: rsb before rs before ts before pairs
    ('rs rsb ts', {}, (32, 32, N, SUBM, BF, True, False), ('rsb', BF, 448)),
    ('rs rsb ts', {}, (32, 32, N, SUBM, BF, False, False), ('pairs', BF, PAIRS)),
    ('rs rsb ts', {}, (32, 32, N, SUBM, X3, False, False), ('rs', X3, 320)),
    ('rs rsb ts', {}, (32, 32, N - 1, SUBM, X3, False, False), ('ts', X3, TS_PLAN)),
    ('rs rsb ts', {}, (32, 48, N, SUBM, X3, False, False), ('ts', X3, TS_PLAN)),
    ('rs rsb ts', {'_ts_plan': None}, (32, 48, N, SUBM, X3, False, False), ('pairs', X3, PAIRS)),
    ('rs rsb ts', {'_EPILOGUE_STATS': True}, (32, 32, N, SUBM, X3, False, True), ('pairs', X3, PAIRS)),
    ('rs rsb ts', {}, (32, 32, N, DOWN, X3, False, False), ('pairs', X3, PAIRS)),
    ('rs rsb ts', {}, (32, 32, N, SUBM, FP, False, False), ('pairs', FP, PAIRS)),
]


@pytest.mark.parametrize('on,patched,args,want', CASES)
def test_conv_route_table(on, patched, args, want, monkeypatch):
    from contextlib import ExitStack
    from unidet3d_amd import sparse
    for name, value in {'_CONV_TS': False, '_CONV_RS': False, '_CONV_RS_BF16': False, '_RS_MIN_ROWS': N, '_RS_MAX_BLOCKS': 8,
                        '_EPILOGUE_STATS': False, '_ts_plan': TS_PLAN, **patched}.items():
        if name == '_ts_plan':
            monkeypatch.setattr(sparse, name, lambda Cs, Cd, n, plan=value: plan)
        else:
            monkeypatch.setattr(sparse, name, value)
    monkeypatch.setattr(sparse, '_plan', lambda Cs, Cd, K, n_dst, rows_kernel=False: PAIRS_ROWS[:2] if rows_kernel else PAIRS[:2])
    for env in ('U3D_RS_H', 'U3D_RSB_H'):
        monkeypatch.delenv(env, raising=False)
    with ExitStack() as stack:              # the public toggles, so that they are shown to reach the flags the route reads
        for t in on.split():
            stack.enter_context({'ts': sparse.conv_ts, 'rs': sparse.conv_rs, 'rsb': sparse.conv_rs_bf16}[t](True))
        assert sparse._conv_route(*args) == want
    assert (sparse._CONV_TS, sparse._CONV_RS, sparse._CONV_RS_BF16) == (False, False, False)


def test_conv_toggles_and_pass_heights_are_read_at_call_time(monkeypatch):
    from unidet3d_amd import sparse
    for name in ('_CONV_TS', '_CONV_RS', '_CONV_RS_BF16', '_EPILOGUE_STATS'):
        monkeypatch.setattr(sparse, name, False)
    monkeypatch.setattr(sparse, '_RS_MIN_ROWS', 1)
    monkeypatch.setattr(sparse, '_plan', lambda *a: PAIRS[:2])
    for setter, flag in ((sparse.set_conv_ts, '_CONV_TS'), (sparse.set_conv_rs, '_CONV_RS'), (sparse.set_conv_rs_bf16, '_CONV_RS_BF16')):
        assert setter(True) is False and getattr(sparse, flag) is True          # returns the previous value, lands in sparse's globals
        assert setter(False) is True and getattr(sparse, flag) is False
    monkeypatch.setenv('U3D_RS_H', '256')
    monkeypatch.setenv('U3D_RSB_H', '384')
    monkeypatch.setattr(sparse, '_CONV_RS', True)                               # set from outside, as the tests and tools do
    monkeypatch.setattr(sparse, '_CONV_RS_BF16', True)
    assert sparse._conv_route(32, 32, 7, SUBM, X3, False, False) == ('rs', X3, 256)
    assert sparse._conv_route(32, 32, 7, SUBM, BF, True, False) == ('rsb', BF, 384)
    with sparse.conv_rs(False):
        assert sparse._conv_route(32, 32, 7, SUBM, X3, False, False) == ('pairs', X3, PAIRS)
    assert sparse._CONV_RS is True


def test_wgrad_stream_state_has_one_owner():
    """The weight-gradient stream mode is ONE binding in wgrad_stream: set through sparse, it is what dense / dense16 consult, and
    setting it back restores it; the per-pass bookkeeping dict sparse re-exports is the module's own object."""
    from unidet3d_amd import dense, dense16, dist, sparse
    from unidet3d_amd import wgrad_stream as WS
    assert dense.WS is WS and dense16.WS is WS and sparse.WS is WS
    assert sparse._ASYNC_DW_SEEN is WS._ASYNC_DW_SEEN
    assert sparse.async_dw_ok is WS.async_dw_ok and sparse.end_of_backward is WS.end_of_backward
    assert sparse.join_wgrad_stream is WS.join_wgrad_stream is dist.join_wgrad_stream
    assert not hasattr(sparse, '_WGRAD_OVERLAP')                 # no second copy a reader could go stale on
    before = WS.mode()
    prev = sparse.set_wgrad_overlap(2)
    try:
        assert prev == before and WS.mode() == 2 and dense.WS.mode() == 2 and dense16.WS.mode() == 2
        assert sparse.set_wgrad_overlap(1) == 2 and WS.mode() == 1
    finally:
        sparse.set_wgrad_overlap(prev)
    assert WS.mode() == before
