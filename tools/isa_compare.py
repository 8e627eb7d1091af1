"""Per-kernel comparison of the device assembly of two builds of the same sources (a refactor must leave each kernel's instruction stream alone).
usage: python tools/isa_compare.py <dir of parent .s> <dir of new .s> [new_name_substring=old_name_substring[,old2] ...]
The .s files come from the build's own command plus --offload-device-only -S (unidet3d_amd.csrc.build.command(src, kind=[...])).
A kernel's text is what lies between its `Begin function` and `End function` markers, without comments, with its own mangled
name replaced by a placeholder and the function index dropped from the .LBB<n>_ and .Lfunc_end<n> labels; section-switch directives
(.text / .section: a template kernel lies in a comdat section of its own) are dropped as well.  A kernel of the new build that has no
namesake in the parent is matched through the `new=old` arguments (substrings of the demangled names; a comma separates two old names
only where no space follows it, so `k<3, false>` is one substring): it replaced that kernel.
One line per kernel of the new build: demangled name, same / differs, VGPR / SGPR / LDS / scratch of parent -> new."""
import glob
import os
import re
import subprocess
import sys


def kernels(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', s, re.S):
        name, meta = m.group(1), m.group(2)
        g = lambda k: (re.search(r'\.amdhsa_' + k + r' (\d+)', meta) or [None, '?'])[1]
        b = re.search(r'; -- Begin function ' + re.escape(name) + r'\n(.*?); -- End function', s, re.S)
        lines = [re.sub(r'\s*;.*', '', l) for l in (b.group(1) if b else '').split('\n')]         # comments name labels by index too
        text = re.sub(r'\.(LBB|Lfunc_end)\d+_?', r'.\1_', '\n'.join(l for l in lines if l.strip() and not re.match(r'\s*\.(text|section)\b', l)).replace(name, '<kernel>'))
        out[name] = (text, '/'.join(g(k) for k in ('next_free_vgpr', 'next_free_sgpr', 'group_segment_fixed_size', 'private_segment_fixed_size')))
    return out


def demangle(names):
    res = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return dict(zip(names, res))


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    renames = [a.split('=', 1) for a in sys.argv[3:]]
    old = {}
    for f in sorted(glob.glob(os.path.join(old_dir, '*.s'))):
        old.update({(os.path.basename(f), k): v for k, v in kernels(f).items()})
    old_dn = demangle([k for _, k in old])
    n_same = n_diff = 0
    print('# kernel | same / differs | VGPR/SGPR/LDS/scratch parent -> new')
    for f in sorted(glob.glob(os.path.join(new_dir, '*.s'))):
        new = kernels(f)
        dn = demangle(list(new))
        for name, (text, res) in new.items():
            refs = [(old.get((os.path.basename(f), name)), '')]
            if refs[0][0] is None:         # renamed: every kernel it replaced, in any file of the parent
                refs = [(v, f'   (replaces {old_dn[k]})') for a, b in renames if a in dn[name]
                        for (_, k), v in old.items() if any(x in old_dn[k] for x in re.split(r',(?! )', b))]
            if not refs:
                print(f'{os.path.basename(f)[:-2]}: {dn[name]} | NEW, nothing to compare | {res}')
                n_diff += 1
            for ref, note in refs:
                same = ref[0] == text
                n_same += same
                n_diff += not same
                print(f"{os.path.basename(f)[:-2]}: {dn[name]} | {'same' if same else 'differs'} | {ref[1]} -> {res}{note}")
    print(f'# {n_same} same, {n_diff} differ')
    return 1 if n_diff else 0


if __name__ == '__main__':
    sys.exit(main())
