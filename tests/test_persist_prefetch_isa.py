"""CPU: the persistent kernel's general loop (csrc/pwv_persist_tasks.inc, MODE 0) requests the next unit's rows between GEMM1 and
GEMM2 and must leave them IN FLIGHT under GEMM2.  What broke that once was a register-allocator join copy: the look-back row's first
chunk was loaded into one register and lived in another, so the wave-uniform fast path of load_x() ended in

    s_waitcnt vmcnt(7)
    v_mov_b32_e32 v229, v98

-- in-order return makes that copy a wait for the next unit's eight own-row loads and the chunk, every unit, in front of GEMM2.  The
compiler's own assembly (gfx950 device code, product flags, no GPU needed) must not show the pattern in any of the eight MODE 0
instantiations; the predicate is checked against an excerpt of the assembly it was written for (tests/golden/)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXCERPT = os.path.join(ROOT, 'tests', 'golden', 'persist_prefetch_parent_isa.txt')
WINDOW = 24      # instructions executed before the wait in which the copied register was loaded

# f16x3 and f32, each plain, packed (VARLEN), streaming (STREAM) and ragged (both): <F32, MODE = 0, ...>
MODE0 = ['_ZN3pwv20stack_persist_kernelILb%dELi0ELb%dELb%dEEEvNS_13PersistParamsE' % (f32, v, s) for f32 in (0, 1) for v, s in ((0, 0), (1, 0), (0, 1))] + \
        ['_ZN3pwv27stack_persist_ragged_kernelILb%dELi0EEEvNS_13PersistParamsE' % f32 for f32 in (0, 1)]


def kernels(text):
    """{mangled name: [instructions and `label:` lines]} of an AMDGPU assembly listing (comments and directives dropped)"""
    out, name, body = {}, None, []
    for line in text.splitlines():
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
        t = line.split(';')[0].strip()
        if not t or (t.startswith('.') and not re.match(r'^\.LBB\w+:$', t)):
            continue
        body.append(t)
    return out


def _vregs(op):
    m = re.match(r'^v\[(\d+):(\d+)\]$', op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r'^v(\d+)$', op)
    return {int(m.group(1))} if m else set()


def join_copies(body, window=WINDOW):
    """[(index, wait, copy)]: every `s_waitcnt ... vmcnt(N)` immediately followed by a v_mov_b32 / v_mov_b64 whose source is a destination
    register of a buffer_load_dwordx4 among the `window` instructions executed before the wait -- on ANY path into it: the compiler lays
    cold blocks out between a load and its use, so "preceding" follows the branches (labels, s_branch / s_cbranch_*), not the listing."""
    labels, ins = {}, []
    for t in body:
        m = re.match(r'^(\.LBB\w+):$', t)
        if m:
            labels[m.group(1)] = len(ins)
        else:
            ins.append(t)
    jumps = {}            # instruction index -> the branches that target it
    for k, t in enumerate(ins):
        m = re.match(r'^s_c?branch\w*\s+(\.LBB\w+)$', t)
        if m and m.group(1) in labels:
            jumps.setdefault(labels[m.group(1)], []).append(k)

    def preds(k):
        p = list(jumps.get(k, []))
        if k > 0 and not re.match(r'^(s_branch|s_endpgm|s_setpc_b64)\b', ins[k - 1]):
            p.append(k - 1)
        return p

    found = []
    for i in range(len(ins) - 1):
        if not re.match(r'^s_waitcnt\b.*\bvmcnt\(\d+\)', ins[i]):
            continue
        m = re.match(r'^v_mov_b(?:32|64)(?:_e32|_e64)?\s+[^,]+,\s*(\S+)$', ins[i + 1])
        src = _vregs(m.group(1)) if m else set()
        if not src:
            continue
        loaded, seen, front = set(), {i}, [i]
        for _ in range(window):
            nxt = []
            for k in front:
                for q in preds(k):
                    if q not in seen:
                        seen.add(q)
                        nxt.append(q)
                        lm = re.match(r'^buffer_load_dwordx4\s+([^,]+),', ins[q])
                        if lm:
                            loaded |= _vregs(lm.group(1))
            front = nxt
        if src & loaded:
            found.append((i, ins[i], ins[i + 1]))
    return found


@pytest.fixture(scope='module')
def assembly():
    from tests.util import kernel_assembly
    return kernels(kernel_assembly('pwv_stack_persist.hip'))


def test_predicate_finds_the_join_copy_in_the_excerpt_it_was_written_for():
    ks = kernels(open(EXCERPT).read())
    assert list(ks) == [MODE0[0]]
    hits = join_copies(ks[MODE0[0]])
    assert [(w, c) for _, w, c in hits] == [('s_waitcnt vmcnt(7)', 'v_mov_b32_e32 v229, v98')], hits
    # (the per-lane select path of that excerpt -- waits followed by v_cndmask_b32 -- is not what the predicate is about)
    # the copy is found through the branch (`s_cbranch_scc0 .LBB18_299`): the chunk's load lies more than 24 LINES above the wait
    assert not join_copies(ks[MODE0[0]], window=8)


def test_predicate_on_synthetic_streams():
    load = 'buffer_load_dwordx4 v[10:13], v1, s[4:7], s8 offen sc1'
    assert join_copies([load, 's_waitcnt vmcnt(0)', 'v_mov_b32_e32 v20, v11'])
    assert join_copies([load, 's_waitcnt vmcnt(2) lgkmcnt(0)', 'v_mov_b64_e32 v[20:21], v[12:13]'])
    assert not join_copies([load, 's_waitcnt vmcnt(0)', 'v_mov_b32_e32 v20, v14'])                   # not a loaded register
    assert not join_copies([load, 's_waitcnt vmcnt(0)', 'v_mov_b32_e32 v20, 0'])                     # a constant fill
    assert not join_copies([load, 's_waitcnt lgkmcnt(0)', 'v_mov_b32_e32 v20, v11'])                 # no vmcnt in the wait
    assert not join_copies([load] + ['s_nop 0'] * WINDOW + ['s_waitcnt vmcnt(0)', 'v_mov_b32_e32 v20, v11'])      # out of the window
    # the load in another block, reached through a branch only
    assert join_copies([load, 's_cbranch_scc0 .LBB0_2', 's_endpgm', '.LBB0_1:'] + ['s_nop 0'] * 40 + ['s_endpgm', '.LBB0_2:', 's_waitcnt vmcnt(0)',
                                                                                                      'v_mov_b32_e32 v20, v10'])


@pytest.mark.parametrize('name', MODE0)
def test_no_wait_and_copy_behind_the_prefetched_rows(assembly, name):
    assert name in assembly, sorted(assembly)
    body = assembly[name]
    assert sum(1 for t in body if t.startswith('buffer_load_dwordx4')) >= 48 and sum(1 for t in body if t.startswith('v_mfma')) >= 100      # (it is the kernel)
    hits = join_copies(body)
    assert not hits, hits
