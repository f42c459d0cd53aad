"""The Adam launches of csrc/optimizer.hip -- one adam_kernel template for every combination of loss scale, clip state and average --
compute, bit for bit, what the eight separate kernels before them computed.

tests/golden/adam_bits_parent.json holds sha256 digests recorded by tests/golden/make_adam_bits.py on the MI355X at the commit before the
kernels were merged into one template.  The tests replay that script's cases (its docstring lists them and says what a digest covers) and
compare: the flat entry points at n = 1, 255, 257, 1000 and steps 1, 2, 1000; the 18 combinations at the reduced architecture over five
calls with a skipped update in the middle; the two full-width groups.  Regenerate the file only at a commit whose results are the ones
to keep."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def bits():
    spec = importlib.util.spec_from_file_location("make_adam_bits", os.path.join(_GOLDEN, "make_adam_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded(bits):
    with open(bits.FIXTURE) as f:
        return json.load(f)


def _compare(got, recorded, prefix, count):
    want = {k: v for k, v in recorded.items() if k.startswith(prefix)}
    assert len(want) == count and sorted(got) == sorted(want), (sorted(got), sorted(want))
    bad = [(k, [i + 1 for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b]) for k in sorted(got) if got[k] != want[k]]
    assert all(len(got[k]) == len(want[k]) for k in got) and not bad, "cases (and the calls in them) whose bits differ from the recorded ones: %r" % bad


def test_flat_entry_points_compute_the_recorded_bits(bits, recorded):
    _compare(bits.run_flat(bits.load_lib()), recorded, "flat/", 36)


def test_reduced_architecture_every_variant_five_calls_with_a_skipped_update_compute_the_recorded_bits(bits, recorded):
    got = bits.run_small(bits.load_lib())
    assert all(len(v) == 5 for v in got.values())
    _compare(got, recorded, "small/", 24)


def test_full_width_groups_compute_the_recorded_bits(bits, recorded):
    got = bits.run_full(bits.load_lib())
    assert all(len(v) == 2 for v in got.values())
    _compare(got, recorded, "full/", 2)
