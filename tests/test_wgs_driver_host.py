"""The sequence of library calls WgsTrio.run() makes, pinned on the CPU (tests/fake_capi.py stands in for the device).

Every case runs the driver on the stand-ins and checks three things: the trace of calls equals the recorded one
(tests/golden/wgs_driver/traces.json), the results equal a direct set computation over the blocks' dictionaries, and
afterwards nothing is alive but the caller's read blocks (and the shard records, where they were asked for).

The fixture is recorded with record() below (python -c "from tests.test_wgs_driver_host import record; record()") --
run by hand, and only to pin a sequence that is known to be right: to re-create it, check out the driver the fixture
was recorded from beside this test, record, and diff."""
import json
import os

import numpy as np
import pytest

from rufus_amd import capi, wgs
from tests import fake_capi as fake

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgs_driver", "traces.json")
K, SIZE, LOWER, MIN_COV, MAX_COV, THRESH = 25, 1 << 20, 2, 5, 30, 1
LO = max(5, MIN_COV)
SWITCHES = ("RFX_TRIO_SORTED", "RFX_MAP_AHEAD", "RFX_WGS_TRACE", "RFX_WGS_INJECT_OOM", "RFX_WGS_FORCE_EXCHANGE",
            "RFX_WGS_OVERLAP")
OOM = "fake: out of device memory"

# name -> what to run.  runs: one dictionary of run() arguments per run() call (n: how many samples it is given);
# exclude / probe: the test fills in an exclude set / the expected hash list; fail: Ctx.fail_finish; raises: what the
# (last) run() must raise; after: attributes of the driver afterwards.
CASES = {
    "binned_p1": dict(n=3, passes=1),
    "binned_p2": dict(n=3, passes=2),
    "binned_p3": dict(n=3, passes=3),
    "sorted_p3": dict(n=3, passes=3, env={"RFX_TRIO_SORTED": "1"}),
    "no_control_binned": dict(n=1, passes=2),
    "no_control_sorted": dict(n=1, passes=2, env={"RFX_TRIO_SORTED": "1"}),
    "exclude_binned": dict(n=2, passes=2, runs=[dict(exclude=True)]),
    "exclude_sorted": dict(n=2, passes=2, env={"RFX_TRIO_SORTED": "1"}, runs=[dict(exclude=True)]),
    "keep_shard_records": dict(n=3, passes=2, runs=[dict(keep_shard_records=True, exclude=True)]),
    "verify_sorted": dict(n=3, passes=2, runs=[dict(verify=True, probe=True)]),
    "verify_binned": dict(n=3, passes=2, runs=[dict(verify="binned", probe=True)]),
    "verify_binned_keep": dict(n=3, passes=2, runs=[dict(verify="binned", keep_shard_records=True)], raises=ValueError),
    "maps_p3_n4": dict(n=4, passes=3, map_budget=1 << 20),
    "maps_p3_n4_ahead": dict(n=4, passes=3, map_budget=1 << 20, env={"RFX_MAP_AHEAD": "1"}),
    "maps_p3_n2": dict(n=2, passes=3, map_budget=1 << 20),
    "maps_p3_n2_ahead": dict(n=2, passes=3, map_budget=1 << 20, env={"RFX_MAP_AHEAD": "1"}),
    "early_p2": dict(n=3, passes=2, early_budget=3500, big=True),
    "early_p2_sorted": dict(n=3, passes=2, early_budget=3500, big=True, env={"RFX_TRIO_SORTED": "1"}),
    "retry_early": dict(n=3, passes=2, early_budget=3500, big=True, env={"RFX_WGS_INJECT_OOM": "0:early:0"},
                        after=dict(passes=2, early_budget=0, map_budget=0)),
    "retry_maps": dict(n=3, passes=2, map_budget=1 << 20, env={"RFX_WGS_INJECT_OOM": "0:maps:0"},
                       after=dict(passes=2, early_budget=0, map_budget=0)),
    "retry_more_passes": dict(n=3, passes=2, fail=(1, "s2", OOM), after=dict(passes=3)),
    "retry_more_passes_sorted": dict(n=3, passes=2, fail=(1, "s2", OOM), env={"RFX_TRIO_SORTED": "1"}, after=dict(passes=3)),
    # (the subject's first count: the attempt holds nothing yet when the error leaves run())
    "error_not_memory": dict(n=3, passes=2, fail=(0, "s0", "fake: invalid argument"), raises=capi.RufusError,
                             after=dict(passes=2)),
    "two_runs_maps": dict(n=3, passes=2, map_budget=1 << 20, runs=[dict(), dict(n=1)]),
    "two_runs_after_retry": dict(n=3, passes=2, early_budget=3500, big=True, env={"RFX_WGS_INJECT_OOM": "0:early:0"},
                                 runs=[dict(), dict(n=2, exclude=True)], after=dict(passes=2, early_budget=0)),
}
# (not in the fixture: the driver the fixture was recorded from kept the subject's store of the pass alive here)
UNPINNED = {"error_not_memory_midpass": dict(n=3, passes=2, fail=(1, "s2", "fake: invalid argument"), raises=capi.RufusError)}


def make_samples(ctx, n_samples, big):
    """n_samples x 2 blocks over 400 keys, and each sample's total count of every key."""
    rng = np.random.default_rng(20260)
    keys = sorted(set(int(x) for x in rng.integers(1, 1 << 50, 400)))
    samples, totals = [], []
    for si in range(n_samples):
        tot = {}
        for key in keys:
            if si == 0:
                tot[key] = int(rng.integers(1, 41))
            elif rng.random() < 0.5:
                tot[key] = int(rng.integers(1, 9))
        first = {key: int(rng.integers(0, c + 1)) for key, c in tot.items()}
        parts = [{k_: c for k_, c in first.items() if c}, {k_: tot[k_] - c for k_, c in first.items() if tot[k_] - c}]
        # (with `big`: the first control's first block is a small one, which ends its early cut)
        samples.append([fake.Block(ctx, "s%db%d" % (si, j), part, n=100 + 7 * j, big=big and (si, j) != (1, 0))
                        for j, part in enumerate(parts)])
        totals.append(tot)
    return samples, totals


def expected(trio, totals, exclude_keys=()):
    """What run() must return, straight from the dictionaries."""
    stores = [{k_: c for k_, c in tot.items() if c >= LOWER} for tot in totals]
    histos = []
    for st in stores:
        h = np.zeros(capi.HISTO_BINS, dtype=np.uint64)
        for c in st.values():
            h[min(c, capi.HISTO_BINS - 1)] += 1
        histos.append(h)
    mutant = {k_: c for k_, c in stores[0].items()
              if LO <= c <= MAX_COV and not any(k_ in st for st in stores[1:]) and k_ not in exclude_keys}
    keys = np.array(sorted(mutant), dtype=np.uint64)
    keys = keys[np.lexsort((keys, trio.pos_of(keys)))]
    return dict(mutant_keys=keys, mutant_counts=np.array([mutant[int(k_)] for k_ in keys], dtype=np.uint32),
                n_records=[len(st) for st in stores], histos=histos, stores=stores)


def run_case(monkeypatch, name):
    """Runs the case, checks results and live handles; returns the trace."""
    case = CASES.get(name) or UNPINNED[name]
    for sw in SWITCHES:
        monkeypatch.delenv(sw, raising=False)
    for sw, val in case.get("env", {}).items():
        monkeypatch.setenv(sw, val)
    ctx = fake.install(monkeypatch)
    samples, totals = make_samples(ctx, case["n"], case.get("big", False))
    blocks = {b.name for s in samples for b in s}
    trio = wgs.WgsTrio(ctx, K, SIZE, LOWER, MIN_COV, MAX_COV, THRESH, passes=case["passes"])
    trio.early_budget, trio.map_budget = case.get("early_budget", 0), case.get("map_budget", 0)
    ctx.fail_finish = case.get("fail")
    plain = expected(trio, totals)
    assert len(plain["mutant_keys"]) >= 8
    excl = fake.Records(ctx, {int(k_): 3 for k_ in plain["mutant_keys"][::3]})
    runs = case.get("runs", [dict()])
    for i, kw in enumerate(runs):
        kw = dict(kw)
        n = kw.pop("n", case["n"])
        want = expected(trio, totals[:n], excl.data if kw.get("exclude") else ())
        if kw.pop("exclude", False):
            kw["exclude"] = [excl]
        if kw.pop("probe", False):
            kw["probe_keys"] = want["mutant_keys"]
        ctx.log("run %d" % i)
        if "raises" in case and i == len(runs) - 1:
            with pytest.raises(case["raises"]) as info:
                trio.run(samples[:n], **kw)
            assert not isinstance(info.value, wgs.GroupFailure)
            assert case.get("fail") is None or str(info.value) == case["fail"][2]
            continue
        out = trio.run(samples[:n], **kw)
        assert np.array_equal(out["mutant_keys"], want["mutant_keys"]) and out["n_mutant"] == len(want["mutant_keys"])
        assert np.array_equal(out["mutant_counts"], want["mutant_counts"]) and out["mutant_counts"].dtype == np.uint32
        assert out["n_records"] == want["n_records"]
        assert len(out["histos"]) == n and all(np.array_equal(a, b) for a, b in zip(out["histos"], want["histos"]))
        assert len(out["hit_masks"]) == len(samples[0]) and out["n_pulled"] == out["n_pulled_local"] > 0
        if kw.get("verify"):
            v = out["verify"]
            assert all(v[x] == 0 for x in v if x.startswith(("bad_", "dup", "not_"))) and v["probe_count_out_of_range"] == 0
            assert v["sum_counts"] == [sum(st.values()) for st in want["stores"]]
            assert v["probe_found"] == [len(want["mutant_keys"])] + [0] * (n - 1)
            assert ("bad_bin" in v) == (kw["verify"] == "binned")
        kept = out.get("shard_records", [])
        assert ("shard_records" in out) == bool(kw.get("keep_shard_records"))
        assert ctx.live == blocks | {excl.name} | ({trio._store.name} if trio._store is not None else set()) | \
            {r.name for shard in kept for r in shard}
        assert len(kept) == (trio.passes if kw.get("keep_shard_records") else 0) and all(len(s_) == n for s_ in kept)
        for shard in kept:
            for r in shard:
                r.free()
        ctx.log("result: passes %d, binned counts %d, replayed blocks %d, maps ahead %d" %
                (trio.passes, trio.binned_counts, trio.replayed_blocks, trio.maps_ahead))
    for attr, val in case.get("after", {}).items():
        assert getattr(trio, attr) == val, attr
    trio.close()
    excl.free()
    assert ctx.live == blocks, "the driver left handles alive"
    assert ctx.used == 0
    return ctx.trace


@pytest.mark.parametrize("name", sorted(CASES))
def test_driver_sequence(monkeypatch, name):
    trace = run_case(monkeypatch, name)
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    assert trace == want, "first difference at line %d" % next(
        (i for i, (a, b) in enumerate(zip(trace, want)) if a != b), min(len(trace), len(want)))


def test_early_cut_uses_the_room_of_the_subjects_records(monkeypatch):
    """3500 bytes of headroom: the subject's two blocks take 2000, the first control's small block ends its cut, and the
    last control's two blocks (2000) fit only with what the subject's raw records of pass 0 gave back at the strike."""
    trace = run_case(monkeypatch, "early_p2")
    adds = [line.split()[1] for line in trace if ".add " in line]
    # (pass 1 takes the controls in reverse; only the first control's blocks are hashed a second time)
    assert adds == ["s0b0", "s0b1", "s1b0", "s1b1", "s2b0", "s2b1", "s1b0", "s1b1"]


def test_any_error_releases_the_attempt(monkeypatch):
    """An error that is no lack of memory, in the middle of a pass: raised to the caller, and nothing stays alive (run_case
    checks that) -- the last thing freed is the subject's store of that pass."""
    trace = run_case(monkeypatch, "error_not_memory_midpass")
    assert trace[-3:] == ["T5.free", "B4.free", "R1.free"] and "B4 = T4.finish_binned" in trace


def test_plan_steps():
    """The orders the driver's comments promise, as literal lists of (pass, sample)."""
    assert wgs.plan_steps(1, 3, False, False) == [(0, 0), (0, 1), (0, 2)]
    # odd passes take the controls in reverse
    assert wgs.plan_steps(3, 3, False, False) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (1, 1), (2, 0), (2, 1), (2, 2)]
    assert wgs.plan_steps(2, 4, False, False) == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 3), (1, 2), (1, 1)]
    # kept shard records stay in the samples' order
    assert wgs.plan_steps(2, 3, False, True) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    # run maps: subject and first control pass by pass, then each further control through all its passes
    assert wgs.plan_steps(3, 4, True, False) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1),
                                                 (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3)]
    assert wgs.plan_steps(2, 3, True, False) == [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (1, 2)]
    # ... which changes nothing for one control or none
    assert wgs.plan_steps(3, 2, True, False) == wgs.plan_steps(3, 2, False, False) == \
        [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
    assert wgs.plan_steps(2, 1, True, False) == [(0, 0), (1, 0)]


def test_plan_maps_ahead():
    """{step: the sample whose maps it queues}: the step before a sample's first, unless a third sample's maps were alive."""
    assert wgs.plan_maps_ahead(wgs.plan_steps(3, 4, True, False)) == {(0, 0): 1, (2, 1): 2, (2, 2): 3}
    assert wgs.plan_maps_ahead(wgs.plan_steps(2, 3, True, False)) == {(0, 0): 1, (1, 1): 2}
    assert wgs.plan_maps_ahead(wgs.plan_steps(3, 2, True, False)) == {(0, 0): 1}
    assert wgs.plan_maps_ahead(wgs.plan_steps(2, 1, True, False)) == {}
    # pass by pass, the subject's maps live until its last pass: the second control's may not be queued beside the first's
    assert wgs.plan_maps_ahead([(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (1, 1)]) == {(0, 0): 1}
    for steps in (wgs.plan_steps(3, 4, True, False), wgs.plan_steps(4, 6, True, False), wgs.plan_steps(3, 3, False, False)):
        ahead = wgs.plan_maps_ahead(steps)
        for i in range(len(steps)):         # maps alive at step i: queued at or before it, last step not yet past
            alive = {s for at, s in ahead.items() if steps.index(at) <= i <= max(j for j, st in enumerate(steps) if st[1] == s)}
            alive |= {steps[i][1]}
            assert len(alive) <= 2, (steps, i, alive)


def test_candidates_one_interface(monkeypatch):
    """Both wrappers: raw until the first strike (range and strike in one call), raw_bytes, finish() without a control."""
    ctx = fake.install(monkeypatch)
    data, mine = {key: key for key in range(1, 41)}, set()
    for cls, store, per in ((wgs._BinnedCandidates, fake.Binned, 12), (wgs._SortedCandidates, fake.Records, 20)):
        c = cls(ctx, store(ctx, data), 5, 30)
        assert len(c) == 40 and c.raw_bytes == 40 * per
        control, excl = store(ctx, {6: 1, 7: 1, 35: 1}), fake.Records(ctx, {8: 2})
        mine |= {control.name, excl.name}
        c.strike(control)
        assert c.raw_bytes == 0 and len(c) == 24
        c.strike(control)
        keys, counts = c.finish([excl])
        assert keys.tolist() == [5] + list(range(9, 31)) and counts.tolist() == keys.tolist()
        c.free()
        keys, _ = cls(ctx, store(ctx, data), 5, 30).finish([])
        assert keys.tolist() == list(range(5, 31))
    assert ctx.live == mine     # the controls and the exclude sets stay the caller's


def record():
    """Writes the fixture from the driver that is importable now."""
    traces = {}
    for name in sorted(CASES):
        with pytest.MonkeyPatch.context() as mp:
            traces[name] = run_case(mp, name)
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        json.dump(traces, f, indent=0, sort_keys=True)
        f.write("\n")
    print({name: len(t) for name, t in traces.items()})
