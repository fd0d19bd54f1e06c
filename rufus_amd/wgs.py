"""WGS-scale driver of the trio hot path (BASELINE.json configs[2]-[3]: synthetic 30x WGS trio, k = 25).

A sample is a LIST of packed read blocks resident in HBM (a block holds < 2^32 k-mer windows, i.e. about
32 M reads of 150 bp).  A 30x human-size sample has 7.8e10 k-mer instances = 187 GB of super-k-mer
records -- more than fits next to the reads -- so the trio runs in S minimizer-shard passes
(``rfx_count_set_shard``): pass s counts shard s of every sample (all blocks into one table; the partition
is refined chunk by chunk at finish), takes the set difference on the shard (the shard of a k-mer is the
same in every sample), adds up the histograms and frees the shard's records.  The mutant k-mers of all
shards, put back into (pos,key) order, are the hash list; the subject's blocks are then filtered.

Two routes.  A plain run needs of every count the histogram, the number of records and the set difference -- none of
which needs the (pos,key) order of jellyfish's file: the survivors stay grouped by minimizer bin (capi.Binned) and the
controls are struck off bin against bin.  Verified or kept records, a group of ranks: sorted records (capi.Records), as
ever; RFX_TRIO_SORTED=1 forces them (A/B, bisecting).  The run loop sees neither: the subject's store of a pass becomes a
_BinnedCandidates or a _SortedCandidates, which have one interface (strike, finish, raw_bytes, free).

Everything that computes is a C-ABI call into the HIP library; this module only sequences them (the same
sequence the drop-in executables run per sample; tests/test_wgs_driver_host.py pins it).
"""
from __future__ import annotations

import os
import time

import numpy as np

from . import capi
from .dist import revcomp_keys


class _DevMem32:
    """n int32 at a raw device address, for torch.as_tensor (no copy)."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 3,
                                         "strides": None}


def _device_view32(ptr: int, n: int, device):
    import torch
    return torch.as_tensor(_DevMem32(ptr, n), device=device)


class _LibraryCall:
    """fn(*args) on a helper thread (ctypes releases the GIL); .err = what it raised."""

    def __init__(self, fn, *args):
        import threading
        self.err = None
        self._t = threading.Thread(target=self._run, args=(fn, args), daemon=True)

    def _run(self, fn, args):
        try:
            fn(*args)
        except Exception as e:      # carried to the next checkpoint by the caller
            self.err = e

    def start(self):
        self._t.start()

    def join(self):
        self._t.join()


class GroupFailure(capi.RufusError):
    """A step failed on SOME rank of the group and every rank knows it: all of them raise this at the same
    checkpoint, so that none is left waiting in a collective.  retry: the failure was a lack of device memory --
    WgsTrio.run() takes one more pass on every rank and starts over."""

    def __init__(self, msg: str, retry: bool):
        super().__init__(msg)
        self.retry = retry


def _is_out_of_memory(e: BaseException) -> bool:
    return "memory" in str(e).lower() or type(e).__name__ == "OutOfMemoryError"


def shard_cut(q: int, n: int) -> int:
    """First of the 256 virtual top-level minimizer bins of shard q of n (rfx_count_set_shard's cut)."""
    return -(-q * 256 // n)

_EVEN = np.uint64(0x5555555555555555)


def pulled_pairs(mask: np.ndarray, n_reads: int) -> int:
    """Number of pairs (reads 2p, 2p+1) with a hit, from the packed per-read hit mask of a block."""
    m = mask[:(n_reads + 63) // 64]
    return int(np.bitwise_count((m | (m >> np.uint64(1))) & _EVEN).sum())


def plan_passes(n_reads_total: int, read_len: int, k: int, resident_bytes: int, hbm_bytes: int, n_samples: int = 3,
                coverage_hint: float = 30.0, world: int = 1, wide: bool = False) -> int:
    """Smallest number of shard passes whose transients fit beside the resident reads of ONE rank.

    n_reads_total: reads per sample over all ranks.  Per pass, sample and rank: super-k-mer records (8 B per
    ~3 k-mer instances; 1 / (S x world) of the sample -- two copies alive at the peak of an exchange: the
    partition and the receive buffers, which the owner counts in place), the refinement scratch (1/8 of the records), the survivor
    arrays (44 B per surviving k-mer: two partition levels + the records), and the subject's candidate records
    of this pass (20 B each; WgsTrio.run counts the subject first and keeps only them).
    On the binned route of run() the survivors are 12-byte staged entries (the pool is ~1.2 x that) for the subject as
    for the sample being counted, and the second partition level and the records do not exist; the estimate below is
    left as it is -- it is then on the safe side, and the pass count stays what it was."""
    windows = n_reads_total * max(read_len - k + 1, 0)           # per sample
    distinct = windows / max(coverage_hint * (read_len - k + 1) / read_len, 1.0)
    for s in range(1, 257 // world):
        share = s * world
        # bytes of records per k-mer instance: a record (12 B) is a whole super-k-mer -- 5.7 k-mers for k <= 25
        # (window of 11 m-mers), 8 for k = 26 .. 31 (window of 16); until round 3: 8 B per ~3 k-mers
        records = (1.6 if wide else 2.2) * windows / share * (2.0 if world > 1 else 1.0)
        # leaf phase of the last sample of a pass: records + scratch, survivor store, the other samples' records
        # (the controls are struck off the subject's candidates one at a time: one set of 20-byte records stays)
        transient = records * 1.125 + 12.0 * distinct / share * 1.3 + (20.0 if n_samples > 1 else 0.0) * distinct / share
        # (measured on the 30x WGS trio, 1 GPU, of 288 GiB: 219 GB at 5 passes, 238 at 4, 271 at 3 -- which this
        # picks; WgsTrio.run() takes one more pass and starts over should a pass not fit after all)
        if resident_bytes + transient < 0.90 * hbm_bytes:
            return s
    return max(1, 256 // world)


def plan_steps(passes: int, n_samples: int, use_maps: bool, keep_shard_records: bool) -> list:
    """Order of the (pass, sample) steps of a run.  The subject (sample 0) is counted first and only its CANDIDATES stay;
    every control then strikes out what it holds and is freed at once: one sample's records alive at a time.
    Plain: pass by pass (odd passes take the controls in reverse: the control counted last in one pass -- whose records of
    the next pass may have been cut ahead in the room the subject's records left, see WgsTrio._attempt -- is the first
    control of the next; kept shard records stay in the samples' order).  With run maps: subject and first control pass by
    pass, then every further control through all its passes at once -- the candidates a shard has left after the first control
    are few, so they can wait, and never more than two samples' maps are alive (the pool is sized for that: bench.py)."""
    P, ns = passes, n_samples
    if use_maps and ns > 2:
        return [(sh, si) for sh in range(P) for si in (0, 1)] + [(sh, si) for si in range(2, ns) for sh in range(P)]
    return [(sh, si) for sh in range(P)
            for si in (list(range(ns)) if sh % 2 == 0 or keep_shard_records else [0] + list(range(ns - 1, 0, -1)))]


def plan_maps_ahead(steps) -> dict:
    """Maps made ahead, {step: sample}: the step before a sample's FIRST step queues that sample's maps -- if the store has
    room for them then (two samples' maps fit: the step must come after the last step of the sample before the previous
    one, whose maps go with its last pass).
    (opt-in, RFX_MAP_AHEAD=1: measured at W it buys nothing -- 1943 against 1941 ms per step --: the hashing launch holds
    414 of a SIMD's 512 registers, the replay and partition workgroups of the first stream do not fit beside it, and the
    two streams take turns instead of sharing the CUs)"""
    first, last_of = {}, {}
    for i, (_, si) in enumerate(steps):
        first.setdefault(si, i)
        last_of[si] = i
    order = sorted(first, key=first.get)
    ahead = {}
    for n, si in enumerate(order[1:], 1):
        at = first[si] - 1                          # the step that queues them
        if n >= 2 and at <= last_of[order[n - 2]]:
            continue                                # (three samples' maps would be alive)
        ahead[steps[at]] = si
    return ahead


class _BinnedCandidates:
    """The subject's candidates of one pass.  They start raw: the subject's store as its count left it (now this object's),
    the count range min_count .. max_count yet to be applied.  strike(control's store; it stays the caller's): the first
    one applies the range and strikes bin against bin in ONE pass over the subject's staged survivors (capi.binned_strike);
    what is left is a short list (capi.Candidates), and every further control is looked up in it, in place.
    finish(exclude) -> (keys, counts): the range alone if no control came, the exclude sets, the read-out; frees itself.
    raw_bytes: what the first strike gives back, 0 after it."""
    entry_bytes = 12        # a staged survivor

    def __init__(self, ctx, store, min_count: int, max_count: int):
        self.ctx, self._h, self._range = ctx, store, (min_count, max_count)

    def __len__(self):
        return len(self._h)

    @property
    def raw_bytes(self) -> int:
        return len(self._h) * self.entry_bytes if self._range else 0

    def _becomes(self, struck):
        self._h.free()
        self._h, self._range = struck, None

    def strike(self, control):
        if self._range:
            self._becomes(capi.binned_strike(self.ctx, self._h, control, *self._range))
        else:
            self._h.strike(control)

    def finish(self, exclude):
        if self._range:
            self.strike(None)
        for ex in exclude:
            self._h.strike_records(ex)
        out = self._h.keys_counts()
        self.free()
        return out

    def free(self):
        if self._h is not None:
            self._h.free()
            self._h = None


class _SortedCandidates(_BinnedCandidates):
    """The same of (pos,key)-sorted capi.Records: every strike is a records_subtract, which returns a new set."""
    entry_bytes = 20        # a record: key, count, pos

    def strike(self, *controls):
        self._becomes(capi.records_subtract(self.ctx, self._h, list(controls), *(self._range or ())))

    def finish(self, exclude):
        if self._range:
            self.strike()
        if exclude:
            self.strike(*exclude)
        out = self._h.get()[:2]
        self.free()
        return out


class _Attempt:
    """What one attempt of WgsTrio.run() has computed, and what it still holds on the device."""

    def __init__(self, n_samples: int, passes: int, verify):
        self.histos, self.n_rec = [np.zeros(capi.HISTO_BINS, dtype=np.uint64) for _ in range(n_samples)], [0] * n_samples
        self.keys, self.kcounts = [], []            # the hash list, pass by pass
        self.recs = {sh: [] for sh in range(passes)}    # pass -> its records that are neither struck off nor kept yet
        self.cands, self.kept = {}, []      # pass -> the subject's candidates; keep_shard_records: the finished passes' records
        self.ver = {"bad_order": 0, "bad_pos": 0, "bad_count": 0, "sum_counts": [0] * n_samples,
                    "probe_found": [0] * n_samples, "probe_count_out_of_range": 0,
                    "checksum": [[0, 0] for _ in range(n_samples)]}   # rfx_records_checksum, summed over the shards
        if verify == "binned":
            self.ver.update(bad_bin=0, duplicate=0, not_canonical=0)

    def release(self):
        """A failed attempt: free what it holds (everything is held in one place, so each thing once)."""
        held = [r for recs in list(self.recs.values()) + self.kept for r in recs] + list(self.cands.values())
        self.recs, self.kept, self.cands = {}, [], {}
        for r in held:
            r.free()


class WgsTrio:
    """count x (subject + controls) -> histograms -> hash list -> filter, in minimizer-shard passes."""

    def __init__(self, ctx: capi.Context, k: int, size: int, lower: int, min_cov: int, max_cov: int, thresh: int,
                 passes: int = 1, group=None):
        """group: a torch.distributed process group -- every rank holds ITS blocks of every sample (strong
        scaling of one trio); records travel to the owner of their minimizer bin, see count_shard()."""
        self.ctx, self.k, self.size = ctx, k, size
        self.lsize = capi.ceil_log2(size)
        self.cols = capi.jf_matrix(self.lsize, k)
        self.lower, self.min_cov, self.max_cov, self.thresh = lower, min_cov, max_cov, thresh
        self.passes = passes
        self.group = group
        self.early_budget = 0       # bytes of device memory that may hold records cut ahead for the next shard pass
        self._early, self._early_left, self._early_cost = {}, 0, 0
        self._injected = False      # RFX_WGS_INJECT_OOM has fired (_inject: once per driver)
        # bytes of device memory that may hold RUN MAPS (32 B per read; rfx_runmaps_*): the first shard pass over a block
        # leaves one, the later passes rebuild their records from reads + map instead of hashing the block again
        # (one store for the trio, ONE piece of device memory of that size, kept from run to run: at 90 % of the HBM maps
        # allocated between the transients of a pass left the arena in pieces.)  With maps the passes are ordered so that
        # at most two samples' maps are alive: run().
        self.map_budget = 0
        self._store = None
        self._ahead = {}            # (pass, sample) -> the blocks whose maps that step queues ahead (run())
        self.maps_ahead = 0         # hashing launches queued on the second stream in the last run()
        self.count_wall_s = 0.0     # host wall time inside count_shard() in the last run() (every count ends with a wait)
        self.masks_are_views = False  # run()'s hit masks stay views of the ctx's page-locked read-back buffer (valid until the next run())
        self.replayed_blocks = 0    # blocks added by replay in the last run()
        self.binned_counts = 0      # (sample, pass) counts of the last run() that ended on the binned route (run())
        # bytes of super-k-mer records this rank sent to / received from OTHER ranks in the last run() (the record
        # exchange of count_shard: RCCL all-to-all over xGMI; what stays on the rank is not counted)
        self.exchange_sent = self.exchange_received = 0
        if group is not None:
            import torch.distributed as dist
            self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        else:
            self.world, self.rank = 1, 0
        if self.passes * self.world > 256:
            raise ValueError("passes x ranks must not exceed the 256 virtual minimizer bins")

    def _count_shard_local(self, blocks, shard: int, si, binned: bool = False):
        """One device: the table of this (sample, shard), from run maps (_add_replayed) or from the blocks (_add_cut_ahead).
        binned: the count ends with the survivors grouped by minimizer bin (capi.Binned) instead of sorted records."""
        held = self._early.pop((si, shard), None) if si is not None else None
        if held is not None:
            t, done = held
        else:
            t, done = capi.CountTable(self.ctx, self.k, self.size, True, mode=capi.COUNT_MSP), frozenset()
            if self.passes > 1:
                t.set_shard(shard, self.passes)
        store = self._store if si is not None and self.passes > 1 else None
        try:
            if store is not None:       # (run maps instead of blocks cut ahead: 32 instead of 132 bytes per read)
                self._add_replayed(t, store, blocks, shard, si)
            else:
                self._add_cut_ahead(t, done, blocks, shard, si)
            if binned:
                self.binned_counts += 1
                return t.finish_binned(self.lower, want_histo=True)
            return t.finish(self.lower, want_histo=True)
        finally:
            t.free()

    def _add_replayed(self, t, store, blocks, shard: int, si):
        """The adds of a count with run maps (the last pass drops them)."""
        t.set_runmaps(store)
        t.prepare_maps(blocks)       # (all of them behind ONE wait: 0.75 ms of idle device per block otherwise)
        # Round 6: the maps of the sample that is counted NEXT are hashed on the ctx's second stream while this
        # sample's records are partitioned, refined and sorted on the first (plan_maps_ahead: self._ahead): the hashing
        # launch is bound by the instructions it issues, the partition levels by the memory, and they share a CU.
        nxt_blocks = self._ahead.pop((shard, si), None) if self._ahead else None
        if nxt_blocks:
            self.maps_ahead += t.prefetch_maps(nxt_blocks)
        last = shard == self.passes - 1
        for b in blocks:
            t.add(b)
            if last:
                store.drop(b)
        self.replayed_blocks += t.replayed()
        if shard == 0:
            self._inject("maps", shard)      # (tests: the headroom turns out not to be there)

    def _add_cut_ahead(self, t, done, blocks, shard: int, si):
        """The adds of a count without run maps.  Shard passes hash every block once per pass; with `early_budget` bytes of
        headroom (bench.py: what the device has left beside the peak of a step) the blocks are, as far as that goes, hashed
        ONCE for this shard and the next (rfx_count_set_early): the next shard's records wait in a table of their own
        (self._early) and that pass is given only the other blocks (`done`: those this table holds already)."""
        todo = [i for i in range(len(blocks)) if i not in done]
        ahead = set()
        if si is not None and self.passes > 1 and shard + 1 < self.passes and self._early_left > 0 and not self.map_budget:
            t.set_early(True)
            cost = self._early_cost
            while todo and self._early_left > cost:     # (cost: what the block before took)
                used0, n0 = self.ctx.mem_stats()["used"], t.early_segments()
                i = todo.pop(0)
                t.add(blocks[i])
                if t.early_segments() == n0:            # not a block for the early cut (small, or the shards meet
                    break                               # inside a coarse bin): neither will the others be
                ahead.add(i)
                # (the block's own segment came with it: the early half is the next shard's share of the growth)
                cost = self._early_cost = (self.ctx.mem_stats()["used"] - used0) // 2
                self._early_left -= cost
            t.set_early(False)
            if ahead:
                self._inject("early", shard)     # (tests: the headroom turns out not to be there)
        for i in todo:
            t.add(blocks[i])
        if ahead:       # (the next pass's table is self._early's from birth: whatever fails here, _drop_early() frees it)
            nxt = capi.CountTable(self.ctx, self.k, self.size, True, mode=capi.COUNT_MSP)
            self._early[(si, shard + 1)] = (nxt, frozenset(ahead))
            nxt.set_shard(shard + 1, self.passes)
            nxt.adopt_early(t)

    def _drop_early(self):
        for t, _ in self._early.values():
            t.free()
        self._early = {}
        if self._store is not None:
            self._store.clear()

    def _drop_store(self):
        if self._store is not None:
            self._store.free()
            self._store = None

    def close(self):
        """Give back what the driver holds between runs (the pool of the run maps)."""
        self._drop_early()
        self._drop_store()

    def _local(self) -> bool:
        return self.world == 1 and not (self.group is not None and os.environ.get("RFX_WGS_FORCE_EXCHANGE"))

    def count_shard(self, blocks, shard: int, si=None, binned: bool = False):
        """Records (in (pos,key) order) + histogram of the k-mers of minimizer shard `shard` of `passes` --
        on N ranks: of this rank's 1/N of that shard.  The cut is flat over passes x ranks virtual shards
        (q = shard * N + rank of passes * N), so a pass is a contiguous range of bins split among the ranks:
        every rank partitions ITS blocks restricted to the pass (rfx_count_set_shard(shard, passes)), the
        records of owner g's bins are one contiguous run per segment -> one all_to_all_single per segment
        (RCCL over xGMI), the owner imports the runs and counts complete bins.  No partial counts, no reduce."""
        if self._local():
            return self._count_shard_local(blocks, shard, si, binned)
        t = capi.CountTable(self.ctx, self.k, self.size, True, mode=capi.COUNT_MSP)
        try:
            err = None
            try:        # local work: a failure here is carried to the first checkpoint of the exchange
                if self.passes > 1:
                    t.set_shard(shard, self.passes)
                self._inject("partition", shard)
                # on a group the other blocks are partitioned while the records of the one before travel
                for b in blocks[:1] if self._overlap() else blocks:
                    t.add(b)
            except Exception as e:
                err = e
            return self._exchange_and_count(t, shard, err, blocks)
        finally:
            t.free()

    def _overlap(self) -> bool:
        """Partition block i + 1 while the records of block i travel?  Yes between devices (RCCL over xGMI moves
        ~0.3 TB/s, a fraction of what the partition leaves of the HBM bandwidth); no when the "exchange" is a copy
        inside one device (RFX_WGS_FORCE_EXCHANGE on one rank: the copy runs at HBM speed against the partition's
        scattered stores -- measured: 66-86 ms per round together, 25 + 5 ms one after the other).  RFX_WGS_OVERLAP=0/1
        overrides.  Not measured on several GPUs (a one-GPU box cannot): profiles/r03_exchange_big.txt."""
        ev = os.environ.get("RFX_WGS_OVERLAP")
        return (ev != "0") if ev is not None else self.world > 1

    def checkpoint(self, err=None):
        """All ranks: did the step succeed everywhere?  One 8-byte all-reduce (MIN of 2 = fine, 1 = out of device
        memory, 0 = anything else).  Returns when every rank is fine; otherwise EVERY rank raises GroupFailure here
        (the rank that failed chains its own exception), retry = all failures were a lack of memory."""
        if self.world == 1:
            if err is not None:
                raise err
            return
        import torch
        import torch.distributed as dist
        from .dist import _wire
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        code = 2 if err is None else (1 if _is_out_of_memory(err) else 0)
        t = _wire(torch.tensor([code], dtype=torch.int64, device=dev), self.group)
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=self.group)
        worst = int(t.item())
        if worst == 2:
            return
        what = "out of device memory" if worst == 1 else "a step failed"
        where = f"on this rank ({err})" if err is not None else "on another rank of the group"
        raise GroupFailure(f"{what} {where}", retry=worst == 1) from err

    def _inject(self, stage: str, shard: int):
        """Fault injection for the tests of the agreed retry: RFX_WGS_INJECT_OOM="rank:stage:shard" makes that rank
        fail once with an out-of-memory error at that stage (partition | receive | finish; early: after blocks were cut
        ahead on one device) of that shard."""
        spec = os.environ.get("RFX_WGS_INJECT_OOM")
        if not spec or getattr(self, "_injected", False):
            return
        r, st, sh = spec.split(":")
        if int(r) == self.rank and st == stage and int(sh) == shard:
            self._injected = True
            raise capi.RufusError(f"injected: out of device memory at {stage} of shard {shard}")

    def _exchange_and_count(self, part: capi.CountTable, shard: int, err, blocks):
        """One round per block: the records of block i go to the owners of their bins (RCCL, torch's stream) WHILE
        block i + 1 is partitioned (the library's stream; rfx_count_add waits for a big block's sizes, so it is called
        from a helper thread -- the library is used by one thread at a time: the main thread makes no library call
        between the helper's start and its join).  part holds blocks[0] already (all blocks when _overlap() says no);
        err: what that raised, if anything.
        Checkpoints (see checkpoint()): before the first round, in every round after the receive buffers are
        allocated (before any record travels), and after the owner's count -- a failure between two of them is
        carried to the next one, never into a collective."""
        import torch
        import torch.distributed as dist
        from .dist import _device_view, _wire, exchange_rows
        W, me, Q = self.world, self.rank, self.passes * self.world
        dev = torch.device("cuda", torch.cuda.current_device())
        vb = [shard_cut(shard * W + g, Q) for g in range(W + 1)]       # owners' ranges in virtual bins
        self.checkpoint(err)
        # every rank may hold a different number of blocks: agree on the rounds
        n_seg = torch.tensor([len(blocks)], dtype=torch.int64, device=dev)
        n_seg = _wire(n_seg, self.group)
        dist.all_reduce(n_seg, op=dist.ReduceOp.MAX, group=self.group)
        rounds = int(n_seg.item())
        own = capi.CountTable(self.ctx, self.k, self.size, True, mode=capi.COUNT_MSP)
        trace = os.environ.get("RFX_WGS_TRACE")
        tt = {"segment": 0.0, "meta": 0.0, "alloc": 0.0, "move": 0.0, "join": 0.0, "import": 0.0}

        def lap(what, t0):      # RFX_WGS_TRACE=host: host wall time only (no device synchronisation: the overlap stays)
            if trace:
                if trace != "host":
                    torch.cuda.synchronize(dev)
                tt[what] += time.perf_counter() - t0
            return time.perf_counter()
        helper = None
        overlap = self._overlap()
        try:
            own.set_shard(shard * W + me, Q)
            keep = []
            wide = True             # records = 64-bit word + 32-bit plane: the plane travels in a second all-to-all
            seg_done = 0
            for i in range(rounds):
                ext = None
                seg = None
                d_ext = 0
                t_ = time.perf_counter()
                if err is None and i < len(blocks):
                    try:        # block i's segment, if it made one (waits for its partition)
                        if part.n_segments() > seg_done:
                            seg = part.segment(seg_done)
                            d_ext = part.segment_ext(seg_done) if wide else 0
                            seg_done += 1
                    except Exception as e:
                        err = e
                t_ = lap("segment", t_)
                helper = None
                if seg is not None:
                    d_rec, d_bs, bins, n = seg
                    rec = _device_view(d_rec, n, dev) if n else torch.empty(0, dtype=torch.int64, device=dev)
                    bs_host = _device_view(d_bs, bins + 1, dev).cpu()
                    if wide:
                        ext = (_device_view32(d_ext, n, dev) if n and d_ext else
                               torch.empty(0, dtype=torch.int32, device=dev))
                else:                                   # nothing to send in this round
                    bins = 256
                    rec = torch.empty(0, dtype=torch.int64, device=dev)
                    bs_host = torch.zeros(bins + 1, dtype=torch.int64)
                    if wide:
                        ext = torch.empty(0, dtype=torch.int32, device=dev)
                per = bins // 256
                cuts = bs_host[torch.tensor([v * per for v in vb])]
                send_l = (cuts[1:] - cuts[:-1]).tolist()
                # sizes, then the bin offsets of each destination's range (relative to its run), then the records
                meta_s = _wire(torch.tensor([[send_l[d], bins] for d in range(W)], dtype=torch.int64, device=dev).flatten(),
                               self.group)
                meta_r = torch.empty_like(meta_s)
                dist.all_to_all_single(meta_r, meta_s, group=self.group)
                meta_r = meta_r.view(W, 2).tolist()
                recv_l = [m[0] for m in meta_r]
                off_parts = [bs_host[vb[d] * per:vb[d + 1] * per + 1] - bs_host[vb[d] * per] for d in range(W)]
                off_sl = [p.numel() for p in off_parts]
                off_rl = [(vb[me + 1] - vb[me]) * (m[1] // 256) + 1 for m in meta_r]
                sb = _wire(torch.cat(off_parts).to(dev), self.group)
                rb = torch.empty(sum(off_rl), dtype=torch.int64, device=sb.device)
                dist.all_to_all_single(rb, sb, off_rl, off_sl, group=self.group)
                t_ = lap("meta", t_)
                rr = re_ = None
                try:
                    self._inject("receive", shard)
                    wr = _wire(rec[int(cuts[0]):int(cuts[-1])], self.group)
                    rr = torch.empty(sum(recv_l), dtype=torch.int64, device=wr.device)
                    if wide:
                        we = _wire(ext[int(cuts[0]):int(cuts[-1])], self.group)
                        re_ = torch.empty(sum(recv_l), dtype=torch.int32, device=we.device)
                except Exception as e:
                    err = e
                self.checkpoint(err)        # also carries a failed import / partition of the round before
                t_ = lap("alloc", t_)
                # Only now, with the round's small collectives done: a partition kernel fills every CU for its ~10 ms,
                # and anything queued behind it on the device waits that long -- measured on one GPU: with the helper
                # started before the metadata exchange every one of its two all-to-alls took a block's partition time
                # (16 ms per round, +2.5 s per W trio in 171 rounds).  The bulk transfer can wait; latency cannot.
                if overlap and i + 1 < len(blocks):
                    helper = _LibraryCall(part.add, blocks[i + 1])
                    helper.start()
                per_rec = 12 if wide else 8
                self.exchange_sent += per_rec * (sum(send_l) - send_l[me])
                self.exchange_received += per_rec * (sum(recv_l) - recv_l[me])
                exchange_rows(rr, wr, recv_l, send_l, self.group)
                if wide:
                    exchange_rows(re_, we, recv_l, send_l, self.group)
                    re_ = re_.to(dev)
                if rr.is_cuda:
                    torch.cuda.current_stream(rr.device).synchronize()   # the library runs on its own stream
                rr, rb = rr.to(dev), rb.cpu()
                t_ = lap("move", t_)
                if helper is not None:      # the next block is partitioned (or failed to be): the library is ours again
                    helper.join()
                    err = err or helper.err
                t_ = lap("join", t_)
                # the bin offsets of every source's run go up first, ONE synchronisation of torch's stream covers them
                # all (round 2 waited once per source), then the imports are queued back to back on the library's stream
                ro = bo = 0
                todo = []
                for src in range(W):
                    sbins = meta_r[src][1]
                    sper = sbins // 256
                    loc = rb[bo:bo + off_rl[src]]
                    full = torch.zeros(sbins + 1, dtype=torch.int64)
                    lo = vb[me] * sper
                    full[lo:lo + off_rl[src]] = loc
                    full[lo + off_rl[src]:] = loc[-1]
                    full = full.to(dev, non_blocking=True)
                    run = rr[ro:ro + recv_l[src]]
                    run_e = re_[ro:ro + recv_l[src]] if wide else None
                    todo.append((run, full, run_e, sbins, recv_l[src]))
                    ro += recv_l[src]
                    bo += off_rl[src]
                torch.cuda.synchronize(dev)
                # the owner counts the runs where they landed (rfx_count_adopt_records_dev: no third copy of the shard's
                # records); the receive buffers live until the table is finished
                try:
                    for run, full, run_e, sbins, n_run in todo:
                        if n_run:
                            own.adopt_records_dev(run.data_ptr(), run.numel(), full.data_ptr(), sbins,
                                                  run_e.data_ptr() if wide else 0)
                        keep.append((run, full, run_e))
                except Exception as e:
                    err = e
                del rr
                t_ = lap("import", t_)
            if trace:
                print("[wgs] exchange of shard %d: " % shard + ", ".join(f"{k_} {v * 1e3:.0f} ms" for k_, v in tt.items()), flush=True)
            part.free()                     # the send views were this table's memory
            out = None
            if err is None:
                try:
                    self._inject("finish", shard)
                    out = own.finish(self.lower, want_histo=True)
                    self.ctx.sync()
                except Exception as e:
                    err = e
            keep.clear()
            self.checkpoint(err)
            return out
        finally:
            if helper is not None:      # (left by an exception: nobody else may be inside the library when tables go)
                helper.join()
            own.free()

    def _verify_store(self, ver, rec, si: int, probe_keys):
        """verify: one shard's records (or store) checked where they lie, added up in `ver`."""
        v = rec.verify(self.lower)
        for k_ in v:
            if k_ != "sum_counts":
                ver[k_] += v[k_]
        ver["sum_counts"][si] += v["sum_counts"]
        ver["checksum"][si] = [(a + b) % (1 << 64) for a, b in zip(ver["checksum"][si], rec.checksum())]
        if probe_keys is not None and len(probe_keys):
            got = rec.query(np.asarray(probe_keys, dtype=np.uint64))
            ver["probe_found"][si] += int((got > 0).sum())
            if si == 0:
                ver["probe_count_out_of_range"] += int(((got > 0) & ((got < max(5, self.min_cov)) |
                                                                     (got > self.max_cov))).sum())

    def pos_of(self, keys: np.ndarray) -> np.ndarray:
        """pos = (M * key) & (2^lsize - 1): bit b of the key selects column 2k-1-b."""
        keys = np.asarray(keys, dtype=np.uint64)
        pos = np.zeros(len(keys), dtype=np.uint64)
        c = 2 * self.k
        for b in range(c):
            pos ^= np.where((keys >> np.uint64(b)) & np.uint64(1), self.cols[c - 1 - b], np.uint64(0))
        return pos & np.uint64((1 << self.lsize) - 1) if self.lsize < 64 else pos

    def _attempt(self, st, samples, keep_shard_records, verify, probe_keys, exclude, lap):
        """One attempt of run() with the present `passes` and budgets: every (pass, sample) step, into `st`."""
        self._drop_early()
        self._early_left = int(self.early_budget) if self.world == 1 and not keep_shard_records else 0
        self.replayed_blocks = self.binned_counts = self.maps_ahead = self.exchange_sent = self.exchange_received = 0
        self.count_wall_s = 0.0
        binned = verify == "binned" or (self._local() and not verify and not keep_shard_records and
                                        not os.environ.get("RFX_TRIO_SORTED"))
        candidates = _BinnedCandidates if binned else _SortedCandidates     # (the two routes: the module's docstring)
        use_maps = self.map_budget > 0 and self.world == 1 and self.passes > 1 and not keep_shard_records
        if not use_maps:
            self._drop_store()
        elif self._store is None:
            try:
                self._store = capi.RunMaps(self.ctx, int(self.map_budget), pooled=True)
            except capi.RufusError:         # no room for the pool: the passes hash as before
                self.map_budget, use_maps = 0, False
        steps = plan_steps(self.passes, len(samples), use_maps, keep_shard_records)
        last_step = {sh: i for i, (sh, _) in enumerate(steps)}
        self._ahead = ({step: samples[si] for step, si in plan_maps_ahead(steps).items()}
                       if use_maps and os.environ.get("RFX_MAP_AHEAD") else {})
        for i_step, (sh, si) in enumerate(steps):
            t_c = time.perf_counter()
            rec, h = self.count_shard(samples[si], sh, si, binned)   # (its failures are agreed inside)
            self.count_wall_s += time.perf_counter() - t_c
            st.recs[sh].append(rec)
            st.histos[si] += h
            st.n_rec[si] += len(rec)
            lap(f"pass {sh} sample {si} count ({len(rec)} records)")
            err = None              # the rest of the iteration is local: on a group its failure is
            try:                    # agreed at its end, so that no rank goes on into a collective alone
                if verify:
                    self._verify_store(st.ver, rec, si, probe_keys)
                    lap(f"pass {sh} sample {si} verify")
                if si == 0 and not keep_shard_records:
                    # The subject's records stay as they are until the first control is there: "MinCov <= count <= MaxDepth"
                    # and "not in control 1" are then ONE pass over them (round 4; before, the range alone made a 31 GB copy
                    # of a W shard that the next step read again: 20 ms per pass).  Without any control: at the end.
                    st.cands[sh] = candidates(self.ctx, st.recs[sh].pop(), max(5, self.min_cov), self.max_cov)
                    lap(f"pass {sh} sample {si} kept ({len(rec)})")
                elif not keep_shard_records:
                    # The step's peak is the count of the FIRST control of a pass (the subject's records wait beside it); from
                    # here on the pass runs that much lower, and so may hold that much more of the next pass's records cut ahead
                    # -- provided the samples they belong to are counted BEFORE the first control of that pass (plan_steps
                    # reverses the controls' order on odd passes).  Two passes only: with more, what is held overlaps.
                    cand = st.cands[sh]
                    room = cand.raw_bytes if self.passes == 2 and sh == 0 and self.early_budget > 0 else 0
                    cand.strike(rec)
                    self._early_left += room
                    st.recs[sh].pop().free()
                    lap(f"pass {sh} sample {si} candidates ({len(cand)})")
            except Exception as e:
                err = e
            self.checkpoint(err)    # (one rank: raises err)
            if i_step != last_step[sh]:
                continue
            if keep_shard_records:
                recs = st.recs[sh]
                k_, c_ = capi.unique_to_subject(self.ctx, recs[0], recs[1:] + exclude, self.min_cov, self.max_cov)
                st.kept.append(st.recs.pop(sh))
            else:
                k_, c_ = st.cands[sh].finish(exclude)
                del st.cands[sh]
            lap(f"pass {sh} set difference ({len(k_)} k-mers)")
            st.keys.append(k_)
            st.kcounts.append(c_)

    def _gather(self, st):
        """(keys, counts, histograms, record counts) of an attempt; on a group: the whole hash list, the sums of the rest."""
        keys = np.concatenate(st.keys) if st.keys else np.zeros(0, np.uint64)
        kcounts = np.concatenate(st.kcounts).astype(np.uint32) if st.kcounts else np.zeros(0, np.uint32)
        if self.world == 1:
            return keys, kcounts, st.histos, st.n_rec
        import torch
        from .dist import all_gather_keys
        dev = torch.device("cuda", torch.cuda.current_device())
        kcounts = all_gather_keys(kcounts.astype(np.uint64), dev, self.group).astype(np.uint32)   # (rank by rank, as the keys)
        keys = all_gather_keys(keys, dev, self.group)
        histos = [x.astype(np.uint64) for x in self._group_sum(np.stack(st.histos))]
        return keys, kcounts, histos, self._group_sum(st.n_rec).tolist()

    def _group_sum(self, values) -> np.ndarray:
        """The ranks' sums of an array of integers."""
        values = np.asarray(values, dtype=np.int64)
        if self.world == 1:
            return values
        import torch
        import torch.distributed as dist
        from .dist import _wire
        t = _wire(torch.from_numpy(values).to(torch.device("cuda", torch.cuda.current_device())), self.group)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t.cpu().numpy()

    def _filter(self, blocks, keys, pull: bool = False):
        """The subject's blocks against the hash list: (pairs pulled, the blocks' hit masks, the pulled pairs as a block
        of their own when `pull`, else None)."""
        n_pulled, masks, pulled = 0, [], None
        if len(keys) or pull:
            mset = capi.MutantSet(self.ctx, np.concatenate([keys, revcomp_keys(keys, self.k)]), self.k)
            try:
                # (all the subject's blocks behind one wait: a call per block left the device idle between two blocks)
                if not len(keys):
                    pulled, res = mset.pull_many([], self.thresh, last_base_skipped=True, pairs=True)[0], []
                elif pull:
                    pulled, res = mset.pull_many(blocks, self.thresh, last_base_skipped=True, pairs=True)
                else:
                    res = mset.filter_many(blocks, self.thresh, last_base_skipped=True)
                for b, (mask, _) in zip(blocks, res):
                    n_pulled += pulled_pairs(mask, b.n)
                    # (views of the ctx's page-locked buffer, overwritten by the next run(): copied unless the caller says
                    # it is done with them by then -- bench.py's timed steps)
                    masks.append(mask if self.masks_are_views else mask.copy())
            finally:
                mset.free()
        return n_pulled, masks, pulled

    def run(self, samples, keep_shard_records: bool = False, verify=False, probe_keys=None, exclude=(), pull: bool = False):
        """samples: [subject blocks, control blocks, ...] (lists of capi.ReadBlock).

        out["mutant_keys"] / out["mutant_counts"]: the hash list in (pos, key) order, `kmer` and the subject's `count`
        (runRufus.sh:925-926).  exclude: capi.Records (a count's, or a .Jhash loaded with Records.load / load_fd) whose
        k-mers are struck off after the controls -- runRufus.sh -e.

        pull: the subject's pulled read pairs as a block of their own, selected on the device (rfx_filter_pull) --
        out["pulled"] = {"block": capi.ReadBlock (the caller frees it), "origin_block", "origin_read": index of the
        subject's block and of the read in it, per pulled read}.  On a process group it is the rank's own: the filter is
        local.  Everything else is as without.

        verify: every shard's records are checked where they lie before they are freed (rfx_records_verify: strict
        (pos,key) order, pos == M * key, lower <= count) -> out["verify"]; probe_keys (canonical keys, e.g. the hash
        list of an earlier run): out["verify"]["probe_found"][sample] = how many of them each sample holds.
        verify=True sorts every shard's records for that; verify="binned" stays on the binned route and checks every store
        where it lies (capi.Binned.verify / checksum / query): the same dictionary, bad_order and bad_pos 0, and bad_bin,
        duplicate, not_canonical beside them."""
        if verify == "binned" and (not self._local() or keep_shard_records):
            raise ValueError('verify="binned": one device, no kept shard records')
        trace = os.environ.get("RFX_WGS_TRACE")
        t_last = time.perf_counter()

        def lap(what):
            nonlocal t_last
            if trace:
                self.ctx.sync()
                print(f"[wgs] {what}: {(time.perf_counter() - t_last) * 1e3:.1f} ms", flush=True)
                t_last = time.perf_counter()

        while True:
            st = _Attempt(len(samples), self.passes, verify)
            try:
                self._attempt(st, samples, keep_shard_records, verify, probe_keys, list(exclude), lap)
                break
            except capi.RufusError as e:
                # the pass plan is an estimate: if a pass does not fit after all, take one more pass and start over.
                # On a group only a failure every rank knows of (GroupFailure: raised by all ranks at the same
                # checkpoint of count_shard) can be retried -- all ranks are here then, with the same `passes`.
                agreed = isinstance(e, GroupFailure) and e.retry
                self._drop_early()              # (run maps / early tables of the failed attempt, whatever follows)
                st.release()
                if (self.world > 1 and not agreed) or self.passes >= 64 or (self.passes + 1) * self.world > 256 or \
                        not _is_out_of_memory(e):
                    raise
                self._drop_early()
                if self.world > 1:
                    import torch
                    torch.cuda.empty_cache()    # the receive buffers of the failed pass go back to the driver
                if self.early_budget > 0 or self.map_budget > 0:    # the headroom for run maps / blocks cut ahead was not
                    self._drop_store()
                    self.early_budget = self.map_budget = 0           # there after all: the same passes once more without
                    if trace:
                        print("[wgs] out of device memory: retrying without run maps / blocks cut ahead", flush=True)
                    continue
                self.passes += 1
                if trace:
                    print(f"[wgs] out of device memory: retrying with {self.passes} passes", flush=True)
        keys, kcounts, histos, n_rec = self._gather(st)
        order = np.lexsort((keys, self.pos_of(keys)))
        keys, kcounts = keys[order], kcounts[order]
        lap("hash list order")
        n_pulled_local, masks, pulled = self._filter(samples[0], keys, pull)
        lap("filter")
        out = {"n_mutant": len(keys), "n_pulled_local": n_pulled_local, "mutant_keys": keys, "mutant_counts": kcounts,
               "n_pulled": int(self._group_sum([n_pulled_local])[0]), "n_records": n_rec, "histos": histos, "hit_masks": masks}
        if pull:
            ob, orr = pulled.origin()
            out["pulled"] = {"block": pulled, "origin_block": ob, "origin_read": orr}
        if keep_shard_records:
            out["shard_records"] = st.kept
        if verify:
            ver, n_ = st.ver, len(samples)
            v_ = self._group_sum([ver["bad_order"], ver["bad_pos"], ver["bad_count"], ver["probe_count_out_of_range"]]
                                 + ver["sum_counts"] + ver["probe_found"]).tolist()
            ver.update(bad_order=v_[0], bad_pos=v_[1], bad_count=v_[2], probe_count_out_of_range=v_[3],
                       sum_counts=v_[4:4 + n_], probe_found=v_[4 + n_:4 + 2 * n_])
            out["verify"] = ver
        return out


_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def expected_snv_kmers(sy: capi.Synth, k: int) -> set:
    """Canonical k-mers that carry the alt allele of a planted SNV of the subject (k per SNV)."""
    expect = set()
    for p, ref, alt in sy.snvs():
        ctxt = bytearray(sy.genome(p - k + 1, 2 * k - 1))
        if bytes(ctxt[k - 1:k]) != ref:
            raise AssertionError("generator: the reference base of an SNV is not the genome's")
        ctxt[k - 1:k] = alt
        for i in range(k):
            km = bytes(ctxt[i:i + k])
            expect.add(min(km, km[::-1].translate(_COMP)))
    return expect


def valid_windows_of_text(seq: np.ndarray, k: int) -> int:
    """ACGT-only windows of length k of a (reads x length) uint8 matrix of read text (host arithmetic only)."""
    ok = np.isin(seq, np.frombuffer(b"ACGTacgt", np.uint8))
    run = np.zeros(seq.shape[0], dtype=np.int32)
    tot = 0
    for j in range(seq.shape[1]):
        run = np.where(ok[:, j], run + 1, 0)
        tot += int((run >= k).sum())
    return tot


def snv_allowance(sy: capi.Synth, n_pairs: int, k: int) -> int:
    """How many k-mers may be the subject's alone without being an SNV's: sites where >= 5 of the c reads that cover a base
    carry the SAME substitution -- G * 3 * C(c, 5) * (e / 3)^5 of them (17 at 30x, 660 at 60x for 3.1 Gb and e = 0.5 %),
    up to k k-mers each; three times that plus 30 sites."""
    import math
    cov = max(5, int(round(n_pairs * 2 * sy.read_len / sy.genome_len)))
    sites = sy.genome_len * 3.0 * math.comb(cov, 5) * (sy.err_1024 / 1024.0 / 3.0) ** 5
    return int(k * (3 * sites + 30))


def self_check(ctx: capi.Context, trio: "WgsTrio", samples, sys_, res, n_pairs, min_q: int = 15,
               more_passes: bool = True, sample_pairs: int = 1 << 17, verify=True) -> dict:
    """What must hold at ANY size, checked on the data of a finished run `res` of `trio` on `samples` (bench.py runs
    this after its timed region; tests/test_scale_gpu.py at the full size of BASELINE configs[2]).  Raises
    AssertionError; returns a summary for the bench line.

    1. a second run with every shard's records verified on the device: strict (pos,key) order
       (jf/include/jellyfish/sorted_dumper.hpp:80-112), pos == M * key, every count >= lower; the sum of the counts
       equals sum(i * histo[i]); the same record counts, histograms, hash list and pulled pairs as `res`;
    2. the mutant k-mers: each is held by the subject with MinCov <= count <= MaxDepth and by NO control (looked up
       in every shard of every sample: merge_files.cc:69-155 + CheckJellyHashList.sh:12 semantics), and they are the
       alt-allele k-mers of the planted SNVs (a handful of recurrent sequencing errors aside);
    3. on one rank: one more shard pass (S + 1) gives the same record counts, histograms, hash list and pulled pairs -- and
       the same multiset of (key, count) records (rfx_records_checksum summed over the shards);
    4. a sampled block of the subject counted alone with lower = 1: sum(i * histo[i]) == the number of ACGT-only
       windows, computed on the host from the generator's host twin (text), not from the packed block.
    verify="binned" (self_check_binned): the route a plain run() takes -- in 1. and 3. every store is verified where the count
    left it (every survivor canonical, count >= lower, in its minimizer's bin, there once) and 1. compares the counts too."""
    binned, k = verify == "binned", trio.k
    keys0 = np.asarray(res["mutant_keys"], dtype=np.uint64)
    rv = trio.run(samples, verify=verify, probe_keys=keys0)
    assert not binned or trio.binned_counts == trio.passes * len(samples), "the binned route was left"
    v = rv["verify"]
    assert all(v[x] == 0 for x in ("bad_order", "bad_pos", "bad_count") + (("bad_bin", "duplicate", "not_canonical") if binned else ())), \
        f"{'stores' if binned else 'records'} fail their invariants: {v}"
    assert rv["n_records"] == res["n_records"] and rv["n_pulled"] == res["n_pulled"]
    assert np.array_equal(rv["mutant_keys"], keys0)
    if binned and "mutant_counts" in res:
        assert np.array_equal(rv["mutant_counts"], res["mutant_counts"])
    for si, h in enumerate(rv["histos"]):
        assert np.array_equal(h, res["histos"][si])
        assert int(h[-1]) != 0 or int(sum(int(x) * i for i, x in enumerate(h))) == v["sum_counts"][si], "histogram != records"
        assert int(h.sum()) == rv["n_records"][si]
    assert v["probe_found"][0] == len(keys0) and v["probe_count_out_of_range"] == 0, "a mutant k-mer is not the subject's"
    assert all(x == 0 for x in v["probe_found"][1:]), "a mutant k-mer occurs in a control"
    out = {"records_verified": int(sum(rv["n_records"])),
           "bin_count_canonical_duplicate_violations" if binned else "order_pos_count_violations": 0,
           "mutant_in_subject": int(v["probe_found"][0]), "mutant_in_controls": int(sum(v["probe_found"][1:]))}
    from .tools import keys_to_text
    if sys_[0].n_snv and len(samples) > 1:
        expect = expected_snv_kmers(sys_[0], k)
        got = set(x.encode() for x in keys_to_text(keys0, k))
        assert len(got) == len(keys0)
        extra = got - expect
        out.update(snv_kmers_expected=len(expect), snv_kmers_found=len(got & expect), not_snv_kmers=len(extra))
        out["not_snv_kmers_allowed"] = snv_allowance(sys_[0], n_pairs, k)
        assert len(extra) <= out["not_snv_kmers_allowed"], f"{len(extra)} mutant k-mers are no SNV k-mers"
        if n_pairs * 300 >= 20 * sys_[0].genome_len:      # at >= 20x nearly every SNV k-mer reaches MinCov
            assert len(got & expect) >= 0.9 * len(expect), f"only {len(got & expect)} of {len(expect)} SNV k-mers found"
    if more_passes and trio.world == 1:
        t2 = WgsTrio(ctx, k, trio.size, trio.lower, trio.min_cov, trio.max_cov, trio.thresh, passes=trio.passes + 1)
        try:
            r2 = t2.run(samples, verify=verify)
            assert not binned or t2.binned_counts == t2.passes * len(samples), "the binned route was left"
        finally:
            t2.close()
        assert r2["n_records"] == res["n_records"] and r2["n_pulled"] == res["n_pulled"]
        assert np.array_equal(r2["mutant_keys"], keys0)
        assert all(np.array_equal(a, b) for a, b in zip(r2["histos"], res["histos"]))
        # the same (key, count) pairs, every one of them, from two different cuts of the work (rfx_records_checksum)
        assert r2["verify"]["checksum"] == v["checksum"], "S and S + 1 shard passes do not hold the same records"
        out["passes_compared"] = [trio.passes, t2.passes]
        out["multiset_checksums"] = ["%016x" % c[0] for c in v["checksum"]]
    if sample_pairs:
        n = int(min(sample_pairs, n_pairs))
        first = (n_pairs - n) // 3
        seq, _ = sys_[0].text(first, n)
        want = valid_windows_of_text(seq, k)
        blk = ctx.synth_reads(sys_[0], first, n, min_q, False, True)
        t = capi.CountTable(ctx, k, trio.size)
        try:
            t.add(blk)
            rec, h = t.finish(1, want_histo=True)
            got_w = int(sum(int(x) * i for i, x in enumerate(h)))
            assert int(h[-1]) == 0 and got_w == want, f"sampled block: {got_w} k-mer instances counted, {want} valid windows"
            rec.free()
        finally:
            t.free()
            blk.free()
        out["sampled_block_windows"] = want
    return out


def self_check_binned(ctx: capi.Context, trio: "WgsTrio", samples, sys_, res, n_pairs, more_passes: bool = True) -> dict:
    """Steps 1-3 of self_check() on the route a plain run() takes (verify="binned")."""
    return self_check(ctx, trio, samples, sys_, res, n_pairs, more_passes=more_passes, sample_pairs=0, verify="binned")


def make_sample(ctx: capi.Context, sy: capi.Synth, n_pairs: int, block_pairs: int = 1 << 24, min_q: int = 15,
                want_good: bool = True, first_pair: int = 0, compact: bool = False):
    """Blocks of a synthetic sample, generated on the device (pairs first_pair .. first_pair + n_pairs)."""
    blocks, p = [], first_pair
    while p < first_pair + n_pairs:
        n = min(block_pairs, first_pair + n_pairs - p)
        blocks.append(ctx.synth_reads(sy, p, n, min_q, want_good, compact))
        p += n
    return blocks
