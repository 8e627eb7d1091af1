"""Host-side checks of the native optimizer tail (unidet3d_amd/optim.py, csrc/optim.hip): the C-ABI triple, the size queries, the
argument checks of the entry points (status codes only: nothing is launched) and the no-fallback rule of ``FlatAdamW``."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIM_ENTRIES = ['u3d_optim_adamw', 'u3d_optim_chunk', 'u3d_optim_grad_sumsq', 'u3d_optim_ws_bytes']


def _header():
    return open(os.path.join(ROOT, 'include', 'u3d.h')).read()


def test_header_ctypes_and_library_agree_on_the_optimizer_entries():
    from unidet3d_amd import _lib as L
    from unidet3d_amd.csrc.build import SOURCES, EXTRA
    assert 'optim.hip' in SOURCES and '-ffp-contract=off' in EXTRA['optim.hip']
    src = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r'\b(u3d_[a-z0-9_]+)\s*\(', src)) if n.startswith('u3d_optim_'))
    assert declared == OPTIM_ENTRIES == sorted(n for n in L.PROTOTYPES if n.startswith('u3d_optim_'))
    lib = L.lib()
    for name in OPTIM_ENTRIES:
        assert hasattr(lib, name)
        m = re.search(r'\b' + name + r'\s*\((.*?)\)\s*;', src, flags=re.S)
        params = [p for p in m.group(1).split(',') if p.strip() and p.strip() != 'void']
        assert len(params) == len(L.PROTOTYPES[name][1]), name
    hdr = int(re.search(r'#define\s+U3D_ABI_VERSION\s+(\d+)', _header()).group(1))
    assert hdr == L.ABI_VERSION == lib.u3d_version()


def test_a_library_without_the_optimizer_entries_is_refused(monkeypatch):
    """The entry points were added without a change of U3D_ABI_VERSION (no existing argument list moved), so an older build passes the
    version check: the loader must still refuse it by name instead of failing with AttributeError at the first call."""
    from unidet3d_amd import _lib as L
    L.lib()
    monkeypatch.setattr(L, '_lib', None)
    monkeypatch.setitem(L.PROTOTYPES, 'u3d_optim_not_built', (ctypes.c_int, []))
    with pytest.raises(L.U3DError, match='does not export u3d_optim_not_built'):
        L.lib()


def test_size_queries_run_without_a_gpu():
    from unidet3d_amd import _lib as L
    from unidet3d_amd import optim
    lib = L.lib()
    chunk = int(re.search(r'#define\s+U3D_OPTIM_CHUNK\s+(\d+)', _header()).group(1))
    parts = int(re.search(r'#define\s+U3D_OPTIM_PARTIALS\s+(\d+)', _header()).group(1))
    assert lib.u3d_optim_chunk() == chunk == optim.CHUNK
    assert chunk % 1024 == 0                                # 256 threads x whole four-element groups
    assert lib.u3d_optim_ws_bytes() == 8 * parts and parts <= 1024          # hundreds of partials, not one per chunk


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Status codes on the host side only: every call below must return U3D_EINVAL from the argument checks, which come before the
    launch (there is no GPU in this test, and none of the pointers is ever dereferenced)."""
    from unidet3d_amd import _lib as L
    lib = L.lib()
    EINVAL = -1
    table = ctypes.c_void_p(0x1000)
    ws = ctypes.c_void_p(0x2000)
    m = ctypes.c_void_p(0x3000)
    assert lib.u3d_optim_grad_sumsq(None, 1, 1, ws, None) == EINVAL                 # null table
    assert b'optim_grad_sumsq' in lib.u3d_last_error()
    assert lib.u3d_optim_grad_sumsq(table, -1, 1, ws, None) == EINVAL               # negative count
    assert lib.u3d_optim_grad_sumsq(table, 1, -1, ws, None) == EINVAL
    assert lib.u3d_optim_grad_sumsq(table, 1, 1, None, None) == EINVAL              # no workspace
    args = (0.9, 0.999, 1e-8, 10.0, 1, ws, m, None)
    assert lib.u3d_optim_adamw(None, 1, 1, m, m, *args) == EINVAL
    assert lib.u3d_optim_adamw(table, -1, 1, m, m, *args) == EINVAL
    assert lib.u3d_optim_adamw(table, 1, 1, ctypes.c_void_p(0x3004), m, *args) == EINVAL      # unaligned moment buffers
    assert b'16-byte aligned' in lib.u3d_last_error()
    assert lib.u3d_optim_adamw(table, 1, 1, m, ctypes.c_void_p(0x3008), *args) == EINVAL
    assert lib.u3d_optim_adamw(table, 1, 1, m, None, *args) == EINVAL
    assert lib.u3d_optim_adamw(table, 1, 1, m, m, 0.9, 0.999, 1e-8, 10.0, 0, ws, m, None) == EINVAL          # step counts from 1
    assert lib.u3d_optim_adamw(table, 1, 1, m, m, 0.9, 0.999, 1e-8, 10.0, 1, None, m, None) == EINVAL       # clipping needs the sums
    assert lib.u3d_optim_adamw(table, 0, 0, m, m, 0.9, 0.999, 1e-8, 0.0, 1, None, None, None) == 0          # nothing to do, nothing launched


def test_cpu_parameters_are_refused():
    from unidet3d_amd import FlatAdamW
    from unidet3d_amd._lib import U3DError
    with pytest.raises(U3DError, match='no CPU fallback'):
        FlatAdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-3)


@pytest.mark.parametrize('flag', ['amsgrad', 'maximize', 'capturable'])
def test_unsupported_flags_are_refused(flag):
    from unidet3d_amd import FlatAdamW
    from unidet3d_amd._lib import U3DError
    with pytest.raises(U3DError, match=flag):
        FlatAdamW([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, **{flag: True})


def test_unsupported_parameters_and_groups_are_refused():
    from unidet3d_amd import FlatAdamW
    from unidet3d_amd._lib import U3DError
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(U3DError, match='betas'):
        FlatAdamW([dict(params=p), dict(params=[torch.nn.Parameter(torch.zeros(4))], betas=(0.8, 0.99))])
    with pytest.raises(U3DError):                          # CPU and fp16: refused either way
        FlatAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
    with pytest.raises(ValueError):
        FlatAdamW(p, lr=-1.0)


def test_the_registry_builds_it_from_a_dict():
    import unidet3d_amd
    from unidet3d_amd import optim
    from unidet3d_amd._lib import U3DError
    assert optim.OPTIMIZERS.get('FlatAdamW') is unidet3d_amd.FlatAdamW
    cfg = dict(type='FlatAdamW', params=[torch.nn.Parameter(torch.zeros(4))], lr=2e-4, weight_decay=0.05, max_norm=10)
    # the registry reaches the constructor, which refuses the CPU parameter (tests/test_gpu_optim.py builds one for real)
    with pytest.raises(U3DError, match='no CPU fallback'):
        optim.OPTIMIZERS.build(cfg)
    with pytest.raises(KeyError):
        optim.OPTIMIZERS.build(dict(type='NoSuchOptimizer', params=[]))
