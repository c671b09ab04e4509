"""Compare the instruction streams of the kernels two builds of one HIP source have in common.

    hipcc --offload-arch=gfx950:xnack- -O3 -std=c++17 -Iinclude -I<csrc> --cuda-device-only -S -o old.s <csrc>/pwv_layer_f16.hip   (parent commit)
    ... the same on this tree ... -o new.s
    python tools/isa_compare.py old.s new.s

Prints, per kernel present in both files, the number of instructions and whether the two streams are equal (comments dropped, the
per-function numbering of local labels normalised), then the kernels only one side has.  Exit status 1 if a common kernel differs.
A kernel template that has gained a trailing template parameter is matched to its earlier self where the new argument is `false`
(stack_persist_kernel<F32, MODE, VARLEN> is stack_persist_kernel<F32, MODE, VARLEN, false> of a tree with STREAM).
"""
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r'^(_Z\w+):', line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith('.Lfunc_end'):
            out[name] = body
            name = None
            continue
        text = line.split(';')[0].strip()
        if not text or text.startswith('.') and not text.startswith('.LBB'):
            continue
        body.append(re.sub(r'\.LBB\d+_', '.LBB_', text))
    return out


def main(old, new):
    a, b = kernels(old), kernels(new)
    # (Itanium mangling: a trailing `false` template argument is `Lb0E` in front of the `E`s that close the argument list and the name)
    for n in sorted(set(b) - set(a)):
        m = re.match(r'^(.*)Lb0E(E+v.*)$', n)
        if m and m.group(1) + m.group(2) in a and m.group(1) + m.group(2) not in b:
            b[m.group(1) + m.group(2)] = b.pop(n)
    names = sorted(set(a) & set(b))
    pretty = subprocess.run(['c++filt'] + names, stdout=subprocess.PIPE, text=True).stdout.split('\n') if names else []
    bad = 0
    for n, p in zip(names, pretty):
        ia = [x for x in a[n] if not x.startswith('.LBB')]
        ib = [x for x in b[n] if not x.startswith('.LBB')]
        same = a[n] == b[n]
        bad += not same
        print('%-9s %6d %6d  %s' % ('equal' if same else 'DIFFERENT', len(ia), len(ib), p.split('(')[0]))
    for tag, only in (('only old', set(a) - set(b)), ('only new', set(b) - set(a))):
        for n in sorted(only):
            print('%-9s %s' % (tag, n))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
