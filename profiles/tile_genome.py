"""Recipe of profiles/tile_genome.txt: kernel time of counting a FASTA of long sequences, tiled and untiled.

    python profiles/tile_genome.py ROW [--bases N] [--runs R] [--warmup W] [--tree DIR] [--label NAME]

ROW is one of
    long      the genome as four FASTA sequences (this build: through the tiler; RFX_NO_TILE=1 or a build without it: untiled)
    reads     the same genome cut on the host into 150-base tiles at step 126, given as FASTA records
    switch    uniform reads of 256 ... 16384 bases, tiled (RFX_TILE_SWITCH=0) against RFX_NO_TILE=1
    tilelen   the genome with RFX_TILE_LEN = 128, 150, 160

--tree DIR imports rufus_amd from another checkout (the parent commit's, built there) instead of this one.

The genome is Synth.genome (seeded), k = 25, -C -L 2, one device.  What is reported is the SUM OF KERNEL DURATIONS from
rfx_prof_* (wall time differs by +- 20 % between boxes), per run, with the kernels that took more than
1 % of it.  Every row is a process of its own; the caller gives each its own time limit."""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
K, SIZE, LOWER = 25, 1 << 32, 2


def fasta(names_seqs, width=70):
    out = []
    for name, s in names_seqs:
        out.append(b">" + name + b"\n")
        out.append(b"\n".join(s[i:i + width] for i in range(0, len(s), width)) + b"\n")
    return b"".join(out)


def kernel_ms(ctx, capi, tools, text, label):
    """One count of FASTA `text` as one block; prints the sum of the kernels' durations."""
    seqs = tools.parse_sequences(text)
    blk = ctx.upload(capi.PackedReads.from_reads(seqs, flags=capi.PACK_COUNT))
    ctx.sync()
    ctx.prof(True)
    ctx.prof_reset()
    t0 = time.time()
    t = capi.CountTable(ctx, K, SIZE)
    t.add(blk)
    rec = t.finish(LOWER)
    ctx.sync()
    wall = time.time() - t0
    prof = ctx.prof_dict()
    ctx.prof(False)
    total = sum(ms for ms, _ in prof.values())
    top = sorted(prof.items(), key=lambda kv: -kv[1][0])
    parts = "  ".join(f"{n} {ms:.2f}/{cnt}" for n, (ms, cnt) in top if ms >= 0.01 * total)
    print(f"{label:28s} kernel_ms {total:10.2f}  wall_ms {wall * 1e3:9.1f}  reads {blk.n:9d}  records {len(rec):10d}  "
          f"checksum {rec.checksum()[0]:016x}  | {parts}", flush=True)
    rec.free()
    t.free()
    blk.free()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=("long", "reads", "switch", "tilelen"))
    ap.add_argument("--bases", type=int, default=200_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1, help="unreported counts first (code load, arena growth)")
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from rufus_amd import capi, tools

    sy = capi.Synth.sample(a.bases, 0, n_snv=0, seed=20261019)
    quarter = a.bases // 4
    with capi.Context(0) as ctx:
        if a.row in ("long", "tilelen"):
            text = fasta([(b"seq%d" % i, sy.genome(i * quarter, quarter)) for i in range(4)])
            for r in range(a.warmup):
                kernel_ms(ctx, capi, tools, text, "(warm-up)")
            if a.row == "long":
                for r in range(a.runs):
                    kernel_ms(ctx, capi, tools, text, f"{a.label or 'long'}_{r + 1}")
            else:
                for L in (128, 150, 160):
                    os.environ["RFX_TILE_LEN"] = str(L)
                    for r in range(a.runs):
                        kernel_ms(ctx, capi, tools, text, f"tile_len_{L}_{r + 1}")
        elif a.row == "reads":
            tiles = []
            for i in range(4):
                s = sy.genome(i * quarter, quarter)
                n, step = -(-(len(s) - K + 1) // 126), 126
                tiles += [(b"s%dt%d" % (i, t), s[t * step:t * step + 150]) for t in range(n)]
            text = fasta(tiles, width=150)
            del tiles
            for r in range(a.warmup):
                kernel_ms(ctx, capi, tools, text, "(warm-up)")
            for r in range(a.runs):
                kernel_ms(ctx, capi, tools, text, f"{a.label or 'reads'}_{r + 1}")
        else:
            g = sy.genome(0, a.bases)
            for r in range(a.warmup):
                kernel_ms(ctx, capi, tools, fasta([(b"w", g[:1_000_000])]), "(warm-up)")
            for length in (256, 512, 1024, 2048, 4096, 8192, 16384):
                text = fasta([(b"r%d" % i, g[i:i + length]) for i in range(0, len(g) - length + 1, length)], width=length)
                for name, env in (("tiled", {"RFX_TILE_SWITCH": "0"}), ("untiled", {"RFX_NO_TILE": "1"})):
                    for key in ("RFX_TILE_SWITCH", "RFX_NO_TILE"):
                        os.environ.pop(key, None)
                    os.environ.update(env)
                    for r in range(a.runs):
                        kernel_ms(ctx, capi, tools, text, f"len_{length}_{name}_{r + 1}")


if __name__ == "__main__":
    main()
