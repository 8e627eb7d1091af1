"""Build libu3d_hip.so (gfx950) in-tree with hipcc.  `python -m unidet3d_amd.csrc.build`."""
import concurrent.futures as cf
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SOURCES = ['misc.hip', 'voxelize.hip', 'rulebook.hip', 'spconv.hip', 'spconv_wg.hip', 'spconv_ts.hip', 'spconv_wgrad_rows.hip', 'spconv_wgrad_blk.hip', 'bn.hip', 'pool.hip', 'sparse_pool.hip', 'sparse_bias.hip', 'sparse_sets.hip', 'sparse_dense.hip', 'sparse_scene.hip', 'relu.hip', 'attn.hip', 'attn_x3.hip', 'gemm.hip', 'gemm_b16.hip', 'norm.hip', 'postproc.hip', 'criterion.hip', 'hashidx.hip', 'radix.hip', 'augment.hip', 'targets.hip', 'optim.hip', 'evalmap.hip']
LIB = os.path.join(HERE, 'libu3d_hip.so')
# (no -munsafe-fp-atomics: since round 5 no kernel of the library issues a floating-point atomic -- every reduction has a fixed order)
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-value',
         '-I', os.path.join(ROOT, 'include'), '-I', HERE]


# per-file code generation options
EXTRA = {'spconv.hip': ['-mllvm', '-amdgpu-mfma-vgpr-form'],
         'spconv_wg.hip': ['-mllvm', '-amdgpu-mfma-vgpr-form'],     # MFMA results are consumed by VALU/LDS right away
         'attn_x3.hip': ['-mllvm', '-amdgpu-mfma-vgpr-form'],
         'postproc.hip': ['-ffp-contract=off'],                     # bit-exact against the oracle's operation order
         'augment.hip': ['-ffp-contract=off'],                      # likewise against transforms.py (blur, affine, trilinear lookup)
         'targets.hip': ['-ffp-contract=off'],                      # likewise against get_targets' squared distances
         'optim.hip': ['-ffp-contract=off'],                        # the dwordx4 and the dword path of a row round alike
         'evalmap.hip': ['-ffp-contract=off']}                      # bit-exact against evaluation.boxes_iou_3d's axis-aligned IoU
# (sparse_pool.hip turns contraction off in the source, `#pragma clang fp contract(off)`: its sums round term by term, in offset order;
#  sparse_bias.hip, sparse_sets.hip and sparse_scene.hip likewise)


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return 'hipcc'


def command(source, extra=(), out=None, kind='-c'):
    """THE hipcc command line of one source file of the library: FLAGS, the file's EXTRA, then the caller's `extra` flags.
    `kind` is the output kind (['-c'] object, ['--offload-device-only', '-S'] device assembly, ...); build(), variant
    libraries (`--variant`, tools/build_variant.sh) and ISA comparisons all compile through this one function."""
    kind = [kind] if isinstance(kind, str) else list(kind)
    out = out or os.path.join(HERE, source.replace('.hip', '.o'))
    return [_hipcc(), *FLAGS, *EXTRA.get(source, []), *extra, *kind, os.path.join(HERE, source), '-o', out]


def _deps(src):
    return [src, *glob.glob(os.path.join(HERE, '*.h')), os.path.join(ROOT, 'include', 'u3d.h'), __file__]


def _stale(src, obj):
    return not os.path.exists(obj) or any(os.path.getmtime(d) > os.path.getmtime(obj) for d in _deps(src))


def _compile(jobs, verbose=True):
    with cf.ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
        for cmd, res in zip(jobs, ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), jobs)):
            if verbose and (res.stdout or res.stderr):
                sys.stderr.write(res.stdout + res.stderr)
            if res.returncode != 0:
                raise RuntimeError('hipcc failed: ' + ' '.join(cmd))


def _link(lib, objs):
    res = subprocess.run([_hipcc(), '--offload-arch=gfx950', '-shared', '-fPIC', '-o', lib, *objs], capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError('link failed: ' + res.stdout + res.stderr)


def build(force: bool = False, verbose: bool = True) -> str:
    objs, jobs = [], []
    for s in SOURCES:
        obj = os.path.join(HERE, s.replace('.hip', '.o'))
        objs.append(obj)
        if force or _stale(os.path.join(HERE, s), obj):
            jobs.append(command(s))
    if jobs:
        _compile(jobs, verbose)
    if jobs or not os.path.exists(LIB):
        _link(LIB, objs)
    return LIB


def build_variant(out, sources, extra, tmp):
    """A/B library: `sources` recompiled into `tmp` with the `extra` flags, every other object from the in-tree build."""
    build(verbose=False)
    redo = {s: os.path.join(tmp, s.replace('.hip', '.o')) for s in sources}
    _compile([command(s, extra, o) for s, o in redo.items()])
    _link(out, [redo.get(s, os.path.join(HERE, s.replace('.hip', '.o'))) for s in SOURCES])
    return out


if __name__ == '__main__':
    if '--variant' in sys.argv:         # --variant <out.so> <file.hip[,file2.hip...]> <extra hipcc flags...>
        import tempfile
        a = sys.argv[sys.argv.index('--variant') + 1:]
        with tempfile.TemporaryDirectory() as tmp:
            print(build_variant(a[0], a[1].split(','), a[2:], tmp))
    else:
        print(build(force='--force' in sys.argv))
