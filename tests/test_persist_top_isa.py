"""CPU: the top of a unit of the persistent kernel's general loop (csrc/pwv_persist_tasks.inc, MODE 0) -- everything between the loop
header and GEMM1's first MFMA -- holds no MFMA, and what a wave waits for there is pure loss.  Two defects stood there once, in
every unit and every wave:

  (a) kernel arguments fetched again per unit (`s_load_dword ... 0x78` = p.proj_row_stride, `s_load_dwordx2 ... 0x28` = p.proj[net],
      each behind its own `s_waitcnt lgkmcnt(0)`) on the address path of the P row: under SGPR pressure the compiler rematerialises
      loop-invariant arguments as scalar loads;
  (b) `s_waitcnt vmcnt(0)` in front of the first `v_cvt_pk_f16_f32` of the own rows' split -- the rows were requested a unit earlier,
      but the wait also covers the 16 P loads issued just before and the previous unit's stores.  Three things put it there: settle_top's
      drain (an asm, which nothing ordered behind the register arithmetic of the split), a register join copy with the unfolded
      layer 0's arm, and above all the layer refill: a `global_load ... lds` is a FLAT-encoded instruction that touches LDS and memory,
      and while the compiler knows of one in flight every vector-memory wait it places is vmcnt(0).  It never learned that the refill
      had landed (the drains are asm), so no load of the loop was left in flight across a wait of the compiler's.

The compiler's own assembly (gfx950 device code, product flags, no GPU needed) must show neither, in any of the eight MODE 0
instantiations ((b): in the four split-fp16 ones; the exact-fp32 arithmetic has no split, its first use of the rows is GEMM1's first
MFMA, which needs the P row as well).  The checks follow the branches, not the listing:

  - "the path every unit takes": an instruction is on it iff every way from the loop's header to the block of GEMM1's first MFMA
    passes through its block (the compiler lays cold blocks -- a unit at an utterance start, a streaming boundary unit, the
    unfolded layer 0, a wave that has to wait -- out between them; those are not checked);
  - (a) also looks at every arm between the header and the P loads: which of them runs is decided per launch (a hop that is a power of
    two or not, a condition or none), so none of them is cold;
  - (b) follows every way from the P loads to the first conversion of the split, the unfolded layer 0's arm excepted.

(The packed instantiations had one more scalar load there, of data and not of an argument: the unit's record of pwv_varlen_unit_map, read
when the unit's rows are requested and again at its top.  The top now maps its rows from the four scalars the request has read.)
The predicates are validated against an excerpt of the assembly they were written for (tests/golden/): the parent's general loop."""
import os
import re

import pytest

from tests.test_persist_prefetch_isa import MODE0, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXCERPT = os.path.join(ROOT, 'tests', 'golden', 'persist_top_parent_isa.txt')
F16X3 = [n for n in MODE0 if 'ILb0E' in n]      # the split-fp16 instantiations: only they split their rows (f32 feeds the rows as loaded)

_TERMINAL = re.compile(r'^(s_branch|s_endpgm|s_setpc_b64)\b')
_BRANCH = re.compile(r'^s_c?branch\w*\s+(\.LBB\w+)$')


def blocks(body):
    """(blocks, succ): the basic blocks of a kernel body ([instructions] each, split at labels and behind branches) and the successor
    lists of its control-flow graph."""
    out, label_of = [[]], {}
    for t in body:
        m = re.match(r'^(\.LBB\w+):$', t)
        if m:
            if out[-1]:
                out.append([])
            label_of[m.group(1)] = len(out) - 1
            continue
        out[-1].append(t)
        if _BRANCH.match(t) or _TERMINAL.match(t):
            out.append([])
    if not out[-1]:
        out.pop()
    succ = []
    for k, b in enumerate(out):
        s = []
        last = b[-1] if b else ''
        m = _BRANCH.match(last)
        if m and m.group(1) in label_of:
            s.append(label_of[m.group(1)])
        if not _TERMINAL.match(last) and k + 1 < len(out):
            s.append(k + 1)
        succ.append(s)
    return out, succ


def _sccs(succ):
    """strongly connected components (Tarjan, iterative), as lists of block indices"""
    n, index, low, on, stack, comps, counter = len(succ), {}, {}, set(), [], [], [0]
    for root in range(n):
        if root in index:
            continue
        work = [(root, 0)]
        while work:
            v, i = work.pop()
            if i == 0:
                index[v] = low[v] = counter[0]
                counter[0] += 1
                stack.append(v)
                on.add(v)
            recurse = False
            for k in range(i, len(succ[v])):
                w = succ[v][k]
                if w not in index:
                    work.append((v, k + 1))
                    work.append((w, 0))
                    recurse = True
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            if recurse:
                continue
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on.discard(w)
                    comp.append(w)
                    if w == v:
                        break
                comps.append(comp)
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    return comps


def _mfmas(b):
    return sum(1 for t in b if t.startswith('v_mfma'))


def _ring_stores(b):
    return sum(1 for t in b if t.startswith('buffer_store_dwordx4'))


def _task_loop(body):
    """(blocks, succ, loop, header) of the general task loop: the cycle of the control-flow graph that stores a unit's rows to the ring (eight
    buffer_store_dwordx4, once write-through and once plain) and holds the most MFMAs -- both GEMMs of a unit; the folded layer-0 loop stores
    rows too but has one GEMM, the tail has no ring stores.  Its header is the block of the cycle that is entered from outside it."""
    bl, succ = blocks(body)
    cands = [set(c) for c in _sccs(succ) if len(c) > 1 and sum(_ring_stores(bl[k]) for k in c) >= 8]
    assert cands, 'no task loop found'
    loop = max(cands, key=lambda c: sum(_mfmas(bl[k]) for k in c))
    assert sum(_mfmas(bl[k]) for k in loop) >= 56, 'no task loop found'
    entered = sorted(k for k in loop if any(k in succ[q] for q in range(len(bl)) if q not in loop))
    assert entered, 'the task loop is never entered'
    # (the compiler rotates the loop: the first task enters it behind the exit test; the header is the entry its own back-edges return to)
    back = [k for k in entered if any(k in succ[q] for q in loop)]
    return bl, succ, loop, (back or entered)[0]


def _walk(bl, succ, loop, header, start, skip=None, stop=None):
    """blocks met from `start` on, in breadth-first order, inside the loop, without passing the header again, the block `skip`, or beyond
    a block with an MFMA / the block `stop`"""
    if start == skip:
        return []
    seen, order, front = {start}, [start], [start]
    while front:
        nxt = []
        for k in front:
            if (_mfmas(bl[k]) and stop is None) or k == stop:
                continue
            for q in succ[k]:
                if q in loop and q not in seen and q != skip and q != header:
                    seen.add(q)
                    order.append(q)
                    nxt.append(q)
        front = nxt
    return order


def _top_blocks(body):
    """(blocks, succ, loop, header, [the blocks every unit passes between the header and GEMM1's first MFMA, in execution order]).  GEMM1's first
    MFMA is in the first block with an MFMA that is reached from the header; a block is on the path every unit takes iff that block cannot be
    reached from the header without it."""
    bl, succ, loop, header = _task_loop(body)

    def target_without(skip):
        hits = [k for k in _walk(bl, succ, loop, header, header, skip) if _mfmas(bl[k])]
        return hits[0] if hits else None

    target = target_without(None)
    assert target is not None, 'no MFMA behind the loop header'
    order = _walk(bl, succ, loop, header, header)
    rest = [k for k in order if k != header and (k == target or target_without(k) is None)]
    ordered = [header]
    while rest:      # (blocks every path passes are totally ordered: one comes first iff it reaches all the others)
        first = [k for k in rest if all(q in _walk(bl, succ, loop, header, k) for q in rest)]
        assert first, rest
        ordered.append(first[0])
        rest.remove(first[0])
    return bl, succ, loop, header, ordered


def unit_top(body):
    """The instructions every unit of the general task loop executes between the loop's header and GEMM1's first MFMA, in order."""
    bl, _, _, _, ordered = _top_blocks(body)
    ins = []
    for k in ordered:
        for t in bl[k]:
            if t.startswith('v_mfma'):
                return ins
            ins.append(t)
    return ins


def _p_loads(b):
    return sum(1 for t in b if re.match(r'^(buffer|global)_load_dwordx4', t))


def address_arms(body):
    """The instructions of every block on ANY way from the loop's header to the block that requests the P row (16 loads of 16 bytes): the row
    maps and the P address with all their arms -- which of them a unit takes (a hop that is a power of two or not, a launch with or without a
    condition, ...) is decided per launch, not per unit, so an arm there is not a cold one."""
    bl, succ, loop, header, ordered = _top_blocks(body)
    pl = [k for k in ordered if _p_loads(bl[k]) >= 16]
    assert pl, 'no P row requested in the top'
    region = [k for k in _walk(bl, succ, loop, header, header, stop=pl[0]) if k == pl[0] or pl[0] in _walk(bl, succ, loop, header, k, stop=pl[0])]
    ins = []
    for k in region:
        for t in bl[k]:
            ins.append(t)
            if k == pl[0] and _p_loads([t]) and _p_loads(ins[-16:]) == 16:
                break
    return ins


def scalar_loads(ins):
    """(a): the scalar memory loads among a list of instructions"""
    return [t for t in ins if re.match(r'^s_(buffer_)?load_', t)]


def waits_before_split(body):
    """(b): on every way from the P row's loads to the first v_cvt_pk_f16_f32 (the split of the unit's own rows), the last `s_waitcnt` with a vmcnt
    that is executed (None: none) -- the set of them, sorted.  The ways follow the branches; the one arm that is left out is the unfolded layer 0,
    which rebuilds both rows from four scalars (v_fmac_f32: nothing else between the P loads and the split multiplies) and has to have them all."""
    bl, succ, loop, header, ordered = _top_blocks(body)
    pl = [k for k in ordered if _p_loads(bl[k]) >= 16]
    assert pl, 'no P row requested in the top'
    found, seen = set(), set()
    work = [(pl[0], None, True)]
    while work:
        k, last, first = work.pop()
        ins = bl[k]
        if first:      # (from behind the 16th load on)
            n = [i for i, t in enumerate(ins) if _p_loads([t])][15]
            ins = ins[n + 1:]
        done = False
        for t in ins:
            if t.startswith('v_cvt_pk_f16_f32'):
                found.add(last)
                done = True
                break
            if t.startswith('v_mfma'):
                done = True
                break
            if re.match(r'^s_waitcnt\b.*\bvmcnt\(\d+\)', t):
                last = t
        if done:
            continue
        for q in succ[k]:
            if q in loop and q != header and (q, last) not in seen and not any(t.startswith('v_fmac_f32') for t in bl[q]):
                seen.add((q, last))
                work.append((q, last, False))
    return sorted(found, key=str)


def drains(wait):
    return wait is not None and re.search(r'\bvmcnt\(0\)', wait) is not None


@pytest.fixture(scope='module')
def assembly():
    from tests.util import kernel_assembly
    return kernels(kernel_assembly('pwv_stack_persist.hip'))


def _norm(ins):
    return [re.sub(r'\s+', ' ', t) for t in ins]


def test_predicates_find_both_patterns_in_the_excerpt_they_were_written_for():
    ks = kernels(open(EXCERPT).read())
    assert list(ks) == [MODE0[0]]
    body = ks[MODE0[0]]
    top = unit_top(body)
    # p.proj_row_stride and p.proj[net] (through the kernarg pointer kept in VGPR lanes), each with a wait of its own, in front of the P row
    assert _norm(scalar_loads(top)) == ['s_load_dword s4, s[0:1], 0x78', 's_load_dwordx2 s[4:5], s[4:5], 0x28']
    assert sum(1 for t in top if t.startswith('global_load_dwordx4')) == 16
    k = [i for i, t in enumerate(top) if t.startswith('s_load_')]
    assert all(top[i + 1].startswith('s_waitcnt lgkmcnt(0)') or top[i + 2].startswith('s_waitcnt lgkmcnt(0)') or top[i + 4].startswith('s_waitcnt lgkmcnt(0)')
               for i in k), [top[i:i + 5] for i in k]
    # ... and p.hop_shift on the arm of a hop that is no power of two (hop 80: every unit)
    assert _norm(scalar_loads(address_arms(body))) == ['s_load_dword s4, s[0:1], 0x78', 's_load_dwordx2 s[4:5], s[4:5], 0x28', 's_load_dword s4, s[0:1], 0xc4']
    # every way to the split ends in a drain
    ws = waits_before_split(body)
    assert ws == ['s_waitcnt vmcnt(0)'] and all(drains(w) for w in ws), ws


def test_predicates_on_synthetic_streams():
    mf = 'v_mfma_f32_32x32x16_f16 a[0:15], v[0:3], v[4:7], a[0:15]'
    st = 'buffer_store_dwordx4 v[0:3], v4, s[4:7], s8 offen'
    pl = ['buffer_load_dwordx4 v[%d:%d], v1, s[4:7], s8 offen' % (4 * k, 4 * k + 3) for k in range(16)]

    def loop(head, mid, cold=(), cold2=()):
        """header block `head` (+ the P loads), an arm `cold` in front of the P loads, `mid` and an arm `cold2` behind them, then the GEMMs and the stores"""
        return (['s_nop 0', '.LBB0_1:'] + list(head) + ['s_cbranch_scc1 .LBB0_5', '.LBB0_2:'] + pl + list(mid) + ['s_cbranch_scc1 .LBB0_6', '.LBB0_3:',
                'v_cvt_pk_f16_f32 v1, v2, v3'] + [mf] * 60 + [st] * 8 + ['s_cbranch_scc1 .LBB0_1', 's_endpgm', '.LBB0_5:'] + list(cold) + ['s_branch .LBB0_2',
                '.LBB0_6:'] + list(cold2) + ['s_branch .LBB0_3'])

    b = loop(['s_load_dword s4, s[0:1], 0x78'], ['s_waitcnt vmcnt(0)'])
    assert scalar_loads(unit_top(b)) == ['s_load_dword s4, s[0:1], 0x78'] and waits_before_split(b) == ['s_waitcnt vmcnt(0)']
    # a scalar load on an arm in front of the P loads is not on the path every unit takes, but it is on the address path
    b = loop(['s_nop 1'], ['s_waitcnt vmcnt(16)'], cold=['s_load_dwordx2 s[4:5], s[0:1], 0x28'])
    assert not scalar_loads(unit_top(b)) and scalar_loads(address_arms(b)) == ['s_load_dwordx2 s[4:5], s[0:1], 0x28']
    assert waits_before_split(b) == ['s_waitcnt vmcnt(16)'] and not drains('s_waitcnt vmcnt(16)')
    # ... behind them (a wave that has to wait, a boundary unit) it is neither
    b = loop(['s_nop 1'], ['s_waitcnt lgkmcnt(0)'], cold2=['s_load_dword s4, s[0:1], 0x78'])
    assert not scalar_loads(unit_top(b)) and not scalar_loads(address_arms(b)) and waits_before_split(b) == [None] and not drains(None)
    # a drain on ONE way to the split is found; the unfolded layer 0's arm (the only one that multiplies) is left out
    b = loop(['s_nop 1'], ['s_waitcnt vmcnt(16)'], cold2=['s_waitcnt vmcnt(0)'])
    assert waits_before_split(b) == ['s_waitcnt vmcnt(0)', 's_waitcnt vmcnt(16)']
    b = loop(['s_nop 1'], ['s_waitcnt vmcnt(16)'], cold2=['s_waitcnt vmcnt(0)', 'v_fmac_f32_e32 v66, v98, v141'])
    assert waits_before_split(b) == ['s_waitcnt vmcnt(16)']
    # the top ends at the first MFMA: what stands behind it is not looked at
    b = loop(['s_nop 1'], [])
    assert not scalar_loads(unit_top(b[:b.index(st)] + ['s_load_dword s4, s[0:1], 0x78'] + b[b.index(st):]))


@pytest.mark.parametrize('name', MODE0)
def test_no_scalar_load_in_the_top_of_a_unit(assembly, name):
    assert name in assembly, sorted(assembly)
    body = assembly[name]
    top = unit_top(body)
    assert sum(1 for t in top if t.startswith('buffer_load_dwordx4')) >= 16 and not any(t.startswith('global_load_dwordx4') for t in top), top      # (the P row is requested there)
    loads = scalar_loads(top) + scalar_loads(address_arms(body))
    assert not loads, loads


@pytest.mark.parametrize('name', F16X3)
def test_the_split_does_not_drain_the_memory_queue(assembly, name):
    body = assembly[name]
    assert any(t.startswith('v_cvt_pk_f16_f32') for t in unit_top(body)), 'no split in the top'
    ws = waits_before_split(body)
    assert ws and not any(drains(w) for w in ws), ws
    # the rows were requested a unit ago: all that was issued behind them is the P row, and that is what stays in flight
    assert all(w is not None and int(re.search(r'vmcnt\((\d+)\)', w).group(1)) >= 16 for w in ws), ws
