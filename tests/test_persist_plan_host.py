"""CPU: the plan and the workspace layout of a persistent launch (csrc/pwv_persist_plan.h: plain C++, no device) in a stand-alone
program built with the host sanitizers, against tests/util.persist_plan_restated -- a restatement written from the design, not from
the header -- over a grid of machines, shapes and knobs, and the plan's refusals."""
import itertools
import os
import subprocess

import pytest

from tests.util import persist_plan_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_FIELDS = ('units', 'nwg', 'per_wg', 'last_wg', 'reach_wgs', 'xcd_map', 'tail_reach_wgs', 'unit_mode')
LAYOUT_FIELDS = ('prog_bytes', 'pair_off', 'uprog_off', 'total')

# one case per line of stdin: cus G rows n_layers d0 d1 min_units max_workgroups tail_q tail_dil (the dilations are d0, d1, 1, 1, ...);
# one line of stdout each: `ok` + the eight plan fields + the four layout numbers, or `refused: <the message>`
PROGRAM = r'''
#include <cstdio>
#define PWV_CHECK_ARG(cond, ...) do { if (!(cond)) { printf("refused: "); printf(__VA_ARGS__); printf("\n"); return PWV_EINVAL; } } while (0)
#include "pwv_persist_plan.h"

int main() {
    int cus, G, n_layers, d0, d1, min_units, max_wgs, tail_q, tail_dil;
    long long rows;
    while (scanf("%d %d %lld %d %d %d %d %d %d %d", &cus, &G, &rows, &n_layers, &d0, &d1, &min_units, &max_wgs, &tail_q, &tail_dil) == 10) {
        int dil[pwv::kMaxPLayers + 1];
        for (int j = 0; j <= pwv::kMaxPLayers; ++j) dil[j] = j == 0 ? d0 : (j == 1 ? d1 : 1);
        pwv::PersistPlan pl;
        if (pwv::persist_plan(G, rows, n_layers, dil, cus, max_wgs, min_units, tail_q, tail_dil, pl) != PWV_OK) continue;
        const pwv::PersistLayout l = pwv::persist_layout(G, pl);
        printf("ok %d %d %d %d %d %d %d %d %zu %zu %zu %zu\n", pl.units, pl.nwg, pl.per_wg, pl.last_wg, pl.reach_wgs, pl.xcd_map, pl.tail_reach_wgs,
               pl.unit_mode, l.prog_bytes, l.pair_off, l.uprog_off, l.total);
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def plan_program(tmp_path_factory):
    d = tmp_path_factory.mktemp('persist_plan')
    src, exe = str(d / 'plan.cpp'), str(d / 'plan')
    with open(src, 'w') as f:
        f.write(PROGRAM)
    res = subprocess.run(['g++', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-Werror',
                          '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'parallel-wavenet-vocoder_amd', 'csrc'), src, '-o', exe],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]

    def run(cases):
        text = ''.join(' '.join(str(v) for v in c) + '\n' for c in cases)
        out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = out.stdout.splitlines()
        assert len(lines) == len(cases), (len(lines), len(cases))
        return lines
    return run


def test_plan_and_layout_equal_the_restatement_on_the_grid(plan_program):
    grid = list(itertools.product((256, 8), (1, 2), (1, 32, 33, 1000, 16000, 28704, 160000), (1, 512, 1056), (0, 8), (0, 6), (0, 1)))
    lines = plan_program([(cus, G, rows, 2, 1, dmax, mu, mw, tq, 512) for cus, G, rows, dmax, mu, mw, tq in grid])
    refused = modes = 0
    for (cus, G, rows, dmax, mu, mw, tq), line in zip(grid, lines):
        want = persist_plan_restated(cus, G, rows, dmax, min_units=mu, max_workgroups=mw, tail_q=tq, tail_dil=512)
        if want is None:
            assert line.startswith('refused: persistent stack:'), ((cus, G, rows, dmax, mu, mw, tq), line)
            refused += 1
            continue
        assert line.split() == ['ok'] + [str(want[k]) for k in PLAN_FIELDS + LAYOUT_FIELDS], ((cus, G, rows, dmax, mu, mw, tq), line, want)
        modes += want['unit_mode'] == 2
    # the grid reaches both instantiations; its refusals are the 160000 rows (5000 units) on at most 6 workgroups per net, over 832 units
    # each: (cus, G, max_workgroups) = (256, 1, 6), (256, 2, 6), (8, 1, 6), (8, 2, 0), (8, 2, 6), times 3 dilations, 2 min_units, 2 tails
    assert 0 < modes < len(grid) - refused and refused == 5 * 3 * 2 * 2, (modes, refused)


def test_plan_refusals(plan_program):
    lines = plan_program([(256, 1, 1000, 1, 1, 1, 0, 0, 0, 0),              # n_layers < 2
                          (256, 1, 1000, 2, 1, 0, 0, 0, 0, 0),              # a dilation of 0
                          (1, 2, 1000, 2, 1, 2, 0, 0, 0, 0),                # cus < G
                          (256, 1, 160000, 2, 1, 1 << 17, 0, 0, 0, 0)])     # 4096 units of reach over 20-unit workgroups
    assert lines[0] == 'refused: persistent stack: 2..32 layers per launch, got 1', lines
    assert lines[1] == 'refused: persistent stack: bad dilation', lines
    assert lines[2] == 'refused: persistent stack: 1 CUs for 2 nets', lines
    assert lines[3] == 'refused: persistent stack: dilation 131072 reaches over 205 workgroups (max 60)', lines
