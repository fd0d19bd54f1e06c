"""Plain Python stand-ins for what rufus_amd/wgs.py uses of capi on one device (tests/test_wgs_driver_host.py).

The driver only sequences library calls, so the sequence can be pinned without a device: every stand-in appends one line
to the context's `trace` per constructor, per free() and per method call (the object's name, the method, its arguments --
objects by name), and the context keeps the set of live handles.  __len__, bits and mem_stats() only read and leave no
line.  Any use of a freed handle, and a second free(), fails at once.

The data model: a read block is a {key: count} dictionary, a key's virtual minimizer bin is key & 255 (the same in every
sample, cut into shards by wgs.shard_cut), a table sums the blocks added restricted to its shard, strikes and
subtractions are set operations.  The results are therefore exact and can be compared with a direct set computation."""
import numpy as np

from rufus_amd import capi as real
from rufus_amd import wgs

EARLY_BYTES = 1000      # device memory a big block's early half takes (its own segment takes as much)
_MIX = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def _arg(a):
    if isinstance(a, _Handle):
        return a.name
    if isinstance(a, (list, tuple)):
        return "[" + " ".join(_arg(x) for x in a) + "]"
    if isinstance(a, np.ndarray):
        return "<%d keys>" % len(a)
    return repr(a)


class Ctx:
    """The context, and the record of everything done through it."""

    def __init__(self):
        self.trace, self.live, self.used, self._n = [], set(), 0, {}
        self.fail_finish = None     # (shard, first letter(s) of the blocks' names, message): the next such finish raises

    def log(self, line):
        self.trace.append(line)

    def name(self, prefix):
        self._n[prefix] = self._n.get(prefix, 0) + 1
        return "%s%d" % (prefix, self._n[prefix])

    def sync(self):
        self.log("ctx.sync")

    def mem_stats(self):
        return {"used": self.used, "peak": self.used, "mapped": self.used}


class _Handle:
    prefix = "H"

    def _born(self, ctx, how, name=None):
        self.ctx, self.name = ctx, name or ctx.name(self.prefix)
        ctx.live.add(self.name)
        ctx.log("%s = %s" % (self.name, how))

    def _call(self, method, *args):
        assert self.name in self.ctx.live, f"{self.name}.{method}: the handle was freed"
        self.ctx.log(" ".join(["%s.%s" % (self.name, method)] + [_arg(a) for a in args]))

    def free(self):
        self._call("free")
        self.ctx.live.remove(self.name)


class Block(_Handle):
    """The caller's read block: n reads, {key: count}; big: one the early cut takes."""

    def __init__(self, ctx, name, counts, n=100, big=False):
        self.counts, self.n, self.big = dict(counts), n, big
        self._born(ctx, "Block", name)


class _Store(_Handle):
    """(key, count) pairs: Records and Binned differ in what verify() reports."""
    report = ()

    def __init__(self, ctx, data, how="load"):
        self.data = dict(data)
        self._born(ctx, how)

    def __len__(self):
        return len(self.data)

    def verify(self, lower=0, upper=_M64):
        self._call("verify", lower)
        out = dict.fromkeys(self.report, 0)
        out.update(bad_count=sum(not lower <= c <= upper for c in self.data.values()), sum_counts=sum(self.data.values()))
        return out

    def checksum(self):
        self._call("checksum")
        mix = [(k * _MIX) & _M64 for k in self.data]
        return sum(m * c for m, c in zip(mix, self.data.values())) & _M64, sum(mix) & _M64

    def query(self, keys):
        self._call("query", keys)
        return np.array([self.data.get(int(k), 0) for k in keys], dtype=np.uint32)


def _arrays(data):
    keys = sorted(data)
    return np.array(keys, dtype=np.uint64), np.array([data[k] for k in keys], dtype=np.uint32)


class Records(_Store):
    prefix, report = "R", ("bad_order", "bad_pos")

    def get(self):
        self._call("get")
        keys, counts = _arrays(self.data)
        return keys, counts, np.zeros(len(keys), np.uint64)


class Binned(_Store):
    prefix, report, bits = "B", ("bad_bin", "not_canonical", "duplicate"), 8


class Candidates(_Store):
    prefix = "C"

    def strike(self, control):
        assert isinstance(control, Binned)
        self._call("strike", control)
        assert control.name in self.ctx.live
        self.data = {k: c for k, c in self.data.items() if k not in control.data}

    def strike_records(self, records):
        assert isinstance(records, Records)
        self._call("strike_records", records)
        assert records.name in self.ctx.live
        self.data = {k: c for k, c in self.data.items() if k not in records.data}

    def keys_counts(self):
        self._call("keys_counts")
        return _arrays(self.data)


def _minus(a, others, lo, hi):
    return {k: c for k, c in a.data.items() if lo <= c <= hi and not any(k in o.data for o in others)}


def binned_strike(ctx, subject, control, min_count=0, max_count=0xFFFFFFFF):
    assert isinstance(subject, Binned) and (control is None or isinstance(control, Binned))
    assert subject.name in ctx.live and (control is None or control.name in ctx.live)
    others = [control] if control is not None else []
    return Candidates(ctx, _minus(subject, others, min_count, max_count),
                      "binned_strike %s %s %d %d" % (subject.name, _arg(control), min_count, max_count))


def records_subtract(ctx, a, others, min_count=0, max_count=0xFFFFFFFF):
    assert all(isinstance(r, Records) and r.name in ctx.live for r in [a] + list(others))
    return Records(ctx, _minus(a, others, min_count, max_count),
                   "records_subtract %s %s %d %d" % (a.name, _arg(others), min_count, max_count))


def unique_to_subject(ctx, subject, others, min_cov, max_cov, min_count=5):
    assert all(isinstance(r, Records) and r.name in ctx.live for r in [subject] + list(others))
    ctx.log("unique_to_subject %s %s %d %d" % (subject.name, _arg(others), min_cov, max_cov))
    return _arrays(_minus(subject, others, max(min_cov, min_count), max_cov))


class RunMaps(_Handle):
    prefix = "M"

    def __init__(self, ctx, budget_bytes=0, pooled=False):
        self.maps = set()
        self._born(ctx, "RunMaps %d %r" % (budget_bytes, pooled))

    def drop(self, block):
        self._call("drop", block)
        self.maps.discard(block.name)

    def clear(self):
        self._call("clear")
        self.maps.clear()


class CountTable(_Handle):
    prefix = "T"

    def __init__(self, ctx, k, size, canonical=True, capacity=0, pos_lo=0, pos_hi=0, mode=real.COUNT_AUTO):
        self.shard, self.n_shards, self.early, self.store = 0, 1, False, None
        self.data, self.ahead, self.went_early, self.adopted, self.added = {}, {}, [], (), []
        self.n_replayed = self.bytes = 0
        self._born(ctx, "CountTable")

    def _share(self, block, shard):
        lo, hi = wgs.shard_cut(shard, self.n_shards), wgs.shard_cut(shard + 1, self.n_shards)
        return {k: c for k, c in block.counts.items() if lo <= (k & 255) < hi}

    @staticmethod
    def _sum(into, part):
        for k, c in part.items():
            into[k] = into.get(k, 0) + c

    def set_shard(self, shard, n_shards):
        self._call("set_shard", shard, n_shards)
        self.shard, self.n_shards = shard, n_shards

    def set_early(self, on=True):
        self._call("set_early", on)
        self.early = on

    def early_segments(self):
        self._call("early_segments")
        return len(self.went_early)

    def add(self, block):
        self._call("add", block)
        assert block.name in self.ctx.live
        assert block.name not in self.adopted, f"{block.name} was cut ahead for this shard and is added again"
        self.added.append(block.name)
        self._sum(self.data, self._share(block, self.shard))
        if self.store is not None:
            self.n_replayed += block.name in self.store.maps
            self.store.maps.add(block.name)
        if self.early and block.big:
            self._sum(self.ahead, self._share(block, self.shard + 1))
            self.went_early.append(block.name)
            self.bytes += 2 * EARLY_BYTES
            self.ctx.used += 2 * EARLY_BYTES

    def adopt_early(self, other):
        self._call("adopt_early", other)
        assert (other.shard + 1, other.n_shards) == (self.shard, self.n_shards)
        self._sum(self.data, other.ahead)
        self.adopted, self.bytes = tuple(other.went_early), self.bytes + other.bytes // 2
        other.ahead, other.went_early, other.bytes = {}, [], other.bytes - other.bytes // 2

    def set_runmaps(self, store):
        self._call("set_runmaps", store)
        self.store = store

    def prepare_maps(self, blocks):
        self._call("prepare_maps", blocks)

    def prefetch_maps(self, blocks):
        self._call("prefetch_maps", blocks)
        return len(blocks)

    def replayed(self):
        self._call("replayed")
        return self.n_replayed

    def _finish(self, kind, how, lower):
        self._call(how, lower)
        ff = self.ctx.fail_finish
        if ff and ff[0] == self.shard and all(n.startswith(ff[1]) for n in self.added + list(self.adopted)):
            self.ctx.fail_finish = None
            raise real.RufusError(ff[2])
        kept = {k: c for k, c in self.data.items() if c >= lower}
        histo = np.zeros(real.HISTO_BINS, dtype=np.uint64)
        for c in kept.values():
            histo[min(c, real.HISTO_BINS - 1)] += 1
        return kind(self.ctx, kept, "%s.%s" % (self.name, how)), histo

    def finish(self, lower=0, upper=_M64, want_histo=False):
        return self._finish(Records, "finish", lower)

    def finish_binned(self, lower=0, upper=_M64, want_histo=False):
        return self._finish(Binned, "finish_binned", lower)

    def free(self):
        super().free()
        self.ctx.used -= self.bytes


class MutantSet(_Handle):
    prefix = "S"

    def __init__(self, ctx, fwd_keys, k):
        self._born(ctx, "MutantSet <%d keys>" % len(fwd_keys))

    def filter_many(self, blocks, thresh=1, last_base_skipped=True):
        self._call("filter_many", blocks, thresh)
        return [(np.full((b.n + 63) // 64 or 1, 0x11 * (i + 1), dtype=np.uint64), 0) for i, b in enumerate(blocks)]


def install(monkeypatch):
    """Put the stand-ins in capi's place (jf_matrix and the constants stay the real ones) and return a fresh context."""
    for name in ("CountTable", "Records", "Binned", "Candidates", "RunMaps", "MutantSet", "binned_strike",
                 "records_subtract", "unique_to_subject"):
        monkeypatch.setattr(real, name, globals()[name])
    return Ctx()
