"""Compare the instruction streams of the kernels two builds of one HIP source have in common.

    hipcc --offload-arch=gfx950:xnack- -O3 -std=c++17 -Iinclude -I<csrc> --cuda-device-only -S -o old.s <csrc>/pwv_layer_f16.hip   (parent commit)
    ... the same on this tree ... -o new.s
    python tools/isa_compare.py old.s new.s

Prints, per kernel present in both files, the number of instructions and whether the two streams are equal (comments dropped, the
per-function numbering of local labels normalised), then the kernels only one side has.  The stream does not show a changed LDS size,
register count or scratch size, so the `.amdhsa_*` lines of the kernel's `.amdhsa_kernel` descriptor are compared too: `DIFFERENT (descriptor)`
where only they differ.  Exit status 1 if a common kernel differs in either.
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


def descriptors(path):
    out, name = {}, None
    for line in open(path):
        text = line.split(';')[0].strip()
        m = re.match(r'^\.amdhsa_kernel\s+(\S+)', text)
        if m:
            name = m.group(1)
            out[name] = []
        elif text.startswith('.end_amdhsa_kernel'):
            name = None
        elif name is not None and text.startswith('.amdhsa_'):
            out[name].append(' '.join(text.split()))
    return out


def main(old, new):
    a, b = kernels(old), kernels(new)
    da, db = descriptors(old), descriptors(new)
    # (Itanium mangling: a trailing `false` template argument is `Lb0E` in front of the `E`s that close the argument list and the name)
    for n in sorted(set(b) - set(a)):
        m = re.match(r'^(.*)Lb0E(E+v.*)$', n)
        if m and m.group(1) + m.group(2) in a and m.group(1) + m.group(2) not in b:
            b[m.group(1) + m.group(2)] = b.pop(n)
            db[m.group(1) + m.group(2)] = db.pop(n, None)
    names = sorted(set(a) & set(b))
    pretty = subprocess.run(['c++filt'] + names, stdout=subprocess.PIPE, text=True).stdout.split('\n') if names else []
    bad = 0
    for n, p in zip(names, pretty):
        ia = [x for x in a[n] if not x.startswith('.LBB')]
        ib = [x for x in b[n] if not x.startswith('.LBB')]
        verdict = 'DIFFERENT' if a[n] != b[n] else ('DIFFERENT (descriptor)' if da.get(n) != db.get(n) else 'equal')
        bad += verdict != 'equal'
        print('%-9s %6d %6d  %s' % (verdict, len(ia), len(ib), p.split('(')[0]))
    for tag, only in (('only old', set(a) - set(b)), ('only new', set(b) - set(a))):
        for n in sorted(only):
            print('%-9s %s' % (tag, n))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
