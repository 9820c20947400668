"""dpb_engine_stats pinned entry for entry: tests/golden/launch_counts.json holds (launches, gemm flops, gemm bytes) after every pass of the tiny
tapes of tests/golden/make_golden_launch_counts.py, recorded from the last commit whose engine kept its launch count by hand (a ledger of
`n_launch += ...` statements next to the calls).  The engine now reports what the launch macro counted; this test replays the same tapes and
demands the recorded triples, so the count stays what it was wherever the ledger was right, and flops / bytes stay what they were everywhere.

ALLOW lists the passes where the ledger was wrong, with the recorded and the true launch count (docs/MEASUREMENT_HISTORY.md section 6.8 explains each):
the adjoint of a concat charged two launches whatever it enqueued, but it copies a column window only to an operand that depends on the seed -- in a
pass seeded at a tap the skip half of every up-block concat does not, so each such concat enqueues one kernel.  Flops and bytes have no exceptions.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# "<entry>": {pass index: (recorded launches, launches now)}
ALLOW = {
    # tiny SD net, (32, 64) channels, one layer per block: four up-block concats; all four lie after the mid tap, two after up block 0
    "unet_sd/jvp_between, vjp_between, iterate_between ('mid', 0)->eps bf16": {1: (87, 83), 2: (338, 330)},     # vjp: -4; two iterations: -8
    "unet_sd/jvp_between, vjp_between, iterate_between ('up', 0)->eps bf16": {1: (71, 69), 2: (276, 272)},
    # small DDPM net, three levels with one resnet each: six up-block concats; all six after the mid tap, four after up level 2 (the first to run)
    "unet_ddpm/jvp_between, vjp_between, iterate_between ('mid', 0)->eps bf16": {1: (75, 69), 2: (306, 294)},
    "unet_ddpm/jvp_between, vjp_between, iterate_between ('up', 2)->eps bf16": {1: (55, 51), 2: (224, 216)},
}


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_launch_counts", os.path.join(HERE, "golden", "make_golden_launch_counts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "launch_counts.json")) as fh:
        return json.load(fh)["stats"]


def test_every_group_is_recorded_and_every_exception_names_a_recorded_pass(recorded):
    assert {k.split("/")[0] for k in recorded} == set(G.GROUPS)
    for entry, passes in ALLOW.items():
        for i, (old, new) in passes.items():
            assert recorded[entry][i][0] == old and new != old, (entry, i)


@pytest.mark.parametrize("group", list(G.GROUPS))
def test_stats_reproduce_the_recorded_passes(group, recorded):
    got = G.record(group)
    want = {k: v for k, v in recorded.items() if k.startswith(group + "/")}
    assert sorted(got) == sorted(want)
    bad = []
    for entry, passes in got.items():
        assert len(passes) == len(want[entry]), entry
        for i, ((n, fl, gb), (n0, fl0, gb0)) in enumerate(zip(passes, want[entry])):
            if (fl, gb) != (fl0, gb0) or (n != n0 and (n0, n) != ALLOW.get(entry, {}).get(i)):
                bad.append((entry, i, (n, fl, gb), (n0, fl0, gb0)))
    assert not bad, bad
