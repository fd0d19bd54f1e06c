"""Host: which k_msp_leaf a launch takes (rufus_amd/csrc/rfx_leaf_variant.h msp_leaf_kc, the function msp_leaf() asks),
printed by tests/host/leaf_variant_harness.cpp for every k, segment count and knob, against the rule as stated: the
kernels compiled for k = 25 and k = 31 when the launch has one segment and neither RFX_LEAF_FORCE_MIXED nor
RFX_LEAF_GENERIC is set, the generic kernel otherwise."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lv") / "leaf_variant_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", out,
                           os.path.join(ROOT, "tests", "host", "leaf_variant_harness.cpp")])
    rows = [tuple(int(x) for x in ln.split()) for ln in subprocess.check_output([out], timeout=60).decode().splitlines()]
    return {r[:4]: r[4] for r in rows}


def test_every_combination_takes_the_variant_the_rule_names(table):
    assert len(table) == 18 * 4 * 2 * 2
    for (k, nseg, fm, fg), kc in table.items():
        want = k if k in (25, 31) and nseg == 1 and not fm and not fg else 0
        assert kc == want, (k, nseg, fm, fg, kc)


def test_the_bench_configurations_take_the_compiled_kernels(table):
    assert table[(25, 1, 0, 0)] == 25 and table[(31, 1, 0, 0)] == 31
    assert {table[(k, 1, 0, 0)] for k in (24, 26, 30, 32)} == {0}
    assert table[(25, 3, 0, 0)] == 0 and table[(25, 1, 1, 0)] == 0 and table[(25, 1, 0, 1)] == 0 and table[(31, 2, 0, 0)] == 0
