"""The grid walks visit what they visited: `candidates`, `grown`, rgc_gicpmp_num_candidates (integer sums the walk alone determines) and the bytes of
FastGICPMultiPoints' merged() (fp64 sums in the walk's order) EQUAL tests/golden/fx_walk_census.json, recorded by tests/golden/gen_walk_census.py from
the library before its walks were folded into rgc_nn.h.  The other GPU suites hold those read-outs to lower bounds only; this one holds the walk itself:
the block of cells of a ball, the row gap test, the cube's growth and exits, the two lane-striding rules.  The cases are the designed ones of the four
subsystems (tests/walk_census.py lists the keys)."""
import json
import os

import pytest

import walk_census

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fx_walk_census.json")


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("part", sorted(walk_census.PARTS))
def test_the_walks_equal_the_record(recorded, part):
    got = walk_census.census((part,))
    want = {k: v for k, v in recorded.items() if k.startswith(part + "/")}
    assert want and sorted(got) == sorted(want), (part, sorted(set(got) ^ set(want))[:10])
    bad = [(k, got[k], want[k]) for k in sorted(got) if got[k] != want[k]]
    print(part, len(got), "entries,", len(bad), "differ")
    assert not bad, bad[:10]
