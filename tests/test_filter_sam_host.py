"""CPU-only: the host side of `RUFUS.Filter --sam` (filter half) through tests/host/filter_sam_harness.cpp --
the tool's own main() with the device entry points replaced by host stand-ins -- so that the reader, the helper
threads, the recycling of pieces and the pairing by QNAME across pieces run without a GPU.  Expected bytes: the
two-process route of runRufus.sh:964-967, i.e. the stranded feeder's two FASTQ streams put through the oracle's filter
(and, where the reference filter can read the input, the reference binaries under oracle/_ref).  The real tool is
compared with the same routes in tests/test_cli_gpu.py::test_filter_sam_equals_feeder_plus_filter."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests.conftest import ROOT
from tests.test_cli_host import BIN, REF, make_sam

HARNESS_SRC = os.path.join(ROOT, "tests", "host", "filter_sam_harness.cpp")
HOST_SRC = os.path.join(ROOT, "rufus_amd", "csrc", "rfx_host.cpp")
K, MIN_Q, THRESH = 25, 15, 1


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("samf") / "filter_sam_harness")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", out, HARNESS_SRC, HOST_SRC])
    return out


def _shuffled_sam(rng, n=6000):
    """Records in random order, names seen two, three and four times, IUPAC / lower-case bases, qualities shorter than
    the read: thousands of reads wait across many pieces."""
    alphabet = np.frombuffer(b"ACGT" * 8 + b"Nacgtn" + b"RY", np.uint8)
    recs = []
    for i in range(n):
        times = 2 if i % 97 else (3 if i % 2 else 4)
        for t in range(times):
            L = int(rng.integers(30, 151))
            seq = bytes(rng.choice(alphabet, L))
            qual = rng.integers(55, 75, L if i % 53 else max(1, L - 7), dtype=np.uint8)
            qual[rng.random(len(qual)) < 0.03] = 35                # '#': below MinQ
            flag = int(rng.choice([99, 147, 83, 163, 16, 0, 1040, 65]))
            recs.append(b"\t".join([b"q%d" % i, b"%d" % flag, b"chr%d" % (1 + i % 5), b"%d" % (i + t), b"60", b"*", b"=",
                                     b"1", b"0", seq, bytes(qual), b"XS:i:%d" % t]) + b"\n")
    return b"".join(recs[j] for j in rng.permutation(len(recs)))


def _hash_list(rng, sam, n_lines):
    lines = [ln.split(b"\t") for ln in sam.split(b"\n") if ln.count(b"\t") >= 10]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    kmers = []
    for j in rng.choice(len(lines), n_lines, replace=False):
        sq = lines[j][9]
        ok = [a for a in range(len(sq) - K + 1) if set(sq[a:a + K]) <= set(b"ACGT")]
        for a in (rng.choice(ok, min(3, len(ok)), replace=False) if ok else ()):
            km = sq[int(a):int(a) + K]
            kmers.append(km if rng.random() < 0.5 else km.translate(comp)[::-1])
    assert len(kmers) > 40
    return b"".join(km + b" 9\n" for km in kmers)


def _records(fq):
    ln = fq.split(b"\n")
    assert ln[-1] == b"" and (len(ln) - 1) % 4 == 0
    return [b"\n".join(ln[i:i + 4]) + b"\n" for i in range(0, len(ln) - 1, 4)]


@pytest.mark.parametrize("shape", ["sorted", "shuffled"])
def test_filter_sam_host_side_equals_feeder_plus_filter(harness, tmp_path, shape):
    d = str(tmp_path)
    rng = np.random.default_rng(5)
    sam = make_sam(3000, seed=8) if shape == "sorted" else _shuffled_sam(rng)
    hl = _hash_list(rng, sam, 200 if shape == "sorted" else 1500)
    open(f"{d}/in.sam", "wb").write(sam)
    open(f"{d}/hl", "wb").write(hl)
    # the two-process route: the drop-in feeder (byte-identical to the reference's, tests/test_cli_host.py) ...
    r = subprocess.run(f"{BIN}/PassThroughSamCheck.stranded two.chr two < in.sam > two.log", shell=True, cwd=d,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr
    m1, m2 = (open(f"{d}/two.mate{m}.fastq", "rb").read() for m in (1, 2))
    # ... and the oracle's filter over its two streams
    pulled = oracle.FilterSet(hl).pairs(m1, m2, K, MIN_Q, THRESH)
    r1, r2 = _records(m1), _records(m2)
    want = [b"".join(r[i] for i in pulled) for r in (r1, r2)]
    assert len(pulled) >= 15
    chr_want = open(f"{d}/two.chr", "rb").read()

    def check(stub):
        for m in (1, 2):
            assert open(f"{d}/{stub}.Mutations.Mate{m}.fastq", "rb").read() == want[m - 1], (stub, m)
        assert open(f"{d}/{stub}.chr", "rb").read() == chr_want, stub

    small = dict(os.environ, RFX_INGEST_PIECE="16384")   # hundreds of pieces: waiting records outlive theirs
    runs = [("pipe1", small, "stdin", "1"), ("pipe5", small, "stdin", "5"), ("pipe3big", dict(os.environ), "stdin", "3"),
            ("file3", small, "in.sam", "3"), ("read3", dict(small, RFX_FILTER_NO_MMAP="1"), "in.sam", "3")]
    for stub, env, src, threads in runs:
        r = subprocess.run([harness, "--sam", f"{stub}.chr", "hl", src, stub, str(K), str(MIN_Q), str(THRESH), threads], cwd=d,
                           env=env, input=sam if src == "stdin" else None, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        check(stub)
    if os.path.exists(f"{REF}/RUFUS.Filter") and shape == "sorted":     # (the reference filter needs whole quality lines)
        r = subprocess.run(f"{REF}/PassThroughSamCheck.stranded ref.chr ref < in.sam > ref.log && "
                           f"{REF}/RUFUS.Filter hl ref.mate1.fastq ref.mate2.fastq ref {K} {MIN_Q} {THRESH} 1 > ref.flog",
                           shell=True, cwd=d, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr
        for m in (1, 2):
            assert open(f"{d}/ref.Mutations.Mate{m}.fastq", "rb").read() == want[m - 1]
        assert open(f"{d}/ref.chr", "rb").read() == chr_want


def test_filter_sam_host_side_many_threads_repeated(harness, tmp_path):
    """The same stream ten times with more helpers than cores and pieces of 4 KB: the order of completion of the
    pieces changes from run to run, the outputs must not."""
    d = str(tmp_path)
    rng = np.random.default_rng(9)
    sam = _shuffled_sam(rng, 1500)
    open(f"{d}/hl", "wb").write(_hash_list(rng, sam, 3000))
    env = dict(os.environ, RFX_INGEST_PIECE="4096", RFX_HOST_THREADS="12")
    first = None
    for rep in range(10):
        r = subprocess.run([harness, "--sam", "x.chr", "hl", "stdin", "x", str(K), str(MIN_Q), str(THRESH), "12"], cwd=d, env=env,
                           input=sam, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr
        got = tuple(open(f"{d}/{f}", "rb").read() for f in ("x.Mutations.Mate1.fastq", "x.Mutations.Mate2.fastq", "x.chr"))
        assert got[0].count(b"\n") >= 40
        first = first or got
        assert got == first


@pytest.mark.parametrize("route", ["files", "fifos"])
def test_paired_filter_host_side(harness, tmp_path, route):
    """The paired tool's own threading (two mate readers in lock step, pieces, ordered output: src/RUFUS.Filter.cpp:162-277)
    over the host stand-ins: the pairs the oracle pulls, from files and from two named pipes fed by the stranded feeder."""
    d = str(tmp_path)
    rng = np.random.default_rng(21)
    sam = make_sam(4000, seed=12)
    hl = _hash_list(rng, sam, 300)
    open(f"{d}/in.sam", "wb").write(sam)
    open(f"{d}/hl", "wb").write(hl)
    r = subprocess.run(f"{BIN}/PassThroughSamCheck.stranded two.chr two < in.sam > two.log", shell=True, cwd=d,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr
    m1, m2 = (open(f"{d}/two.mate{m}.fastq", "rb").read() for m in (1, 2))
    pulled = oracle.FilterSet(hl).pairs(m1, m2, K, MIN_Q, THRESH)
    want = [b"".join(r[i] for i in pulled) for r in (_records(m1), _records(m2))]
    assert len(pulled) >= 15
    env = dict(os.environ, RFX_INGEST_PIECE="8192")
    if route == "files":
        r = subprocess.run([harness, "hl", "two.mate1.fastq", "two.mate2.fastq", "out", str(K), str(MIN_Q), str(THRESH), "4"],
                           cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    else:
        os.mkfifo(f"{d}/ff.mate1.fastq")
        os.mkfifo(f"{d}/ff.mate2.fastq")
        feeder = subprocess.Popen(f"{BIN}/PassThroughSamCheck.stranded ff.chr ff < in.sam > ff.log", shell=True, cwd=d)
        r = subprocess.run([harness, "hl", "ff.mate1.fastq", "ff.mate2.fastq", "out", str(K), str(MIN_Q), str(THRESH), "4"],
                           cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert feeder.wait(timeout=60) == 0
    assert r.returncode == 0, r.stderr
    for m in (1, 2):
        assert open(f"{d}/out.Mutations.Mate{m}.fastq", "rb").read() == want[m - 1]


# ---- `--packed` and its fall-backs, and the refusals of every route, through the harnesses -------------------------------
@pytest.fixture(scope="module")
def single_harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ssf") / "filter_single_harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-DRFX_SINGLE_END", "-o", out,
                           os.path.join(ROOT, "tests", "host", "filter_single_harness.cpp"), HOST_SRC])
    return out


@pytest.fixture(scope="module")
def packed_dir(tmp_path_factory):
    """A directory with in.sam, its hash list hl, the SAM-kind cache `jellyfish count --sam CHR --keep-packed cache.bin in.sam`
    leaves (tests/host/jellyfish_harness.cpp, as tests/test_packed_cache_host.py makes it) and two small mate files."""
    from tests.test_jellyfish_host import _build
    d = str(tmp_path_factory.mktemp("packed"))
    jf = _build(f"{d}/jellyfish", ["-O2"])
    sam = make_sam(3000, seed=23)
    open(f"{d}/in.sam", "wb").write(sam)
    open(f"{d}/hl", "wb").write(_hash_list(np.random.default_rng(23), sam, 300))
    r = subprocess.run([jf, "count", "--disk", "-m", "25", "-L", "2", "-s", "100M", "-t", "4", "-C", "--sam", "c.chr", "--keep-packed",
                        "cache.bin", "-o", "c.Jhash", "in.sam"], cwd=d, env=dict(os.environ, RFX_INGEST_PIECE="40000"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr
    for m in (1, 2):
        open(f"{d}/m{m}.fq", "wb").write(b"".join(b"@r%d/%d\n%s\n+\n%s\n" % (i, m, b"ACGTTGCA" * 8, b"I" * 64) for i in range(3)))
    return d


def _run(exe, d, args, **env):
    return subprocess.run([exe] + args, cwd=d, env=dict(os.environ, RFX_INGEST_PIECE="40000", **env), stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=300)


def _outputs(d, stub):
    return tuple(open(f"{d}/{stub}{f}", "rb").read() for f in (".Mutations.Mate1.fastq", ".Mutations.Mate2.fastq", ".chr"))


def _left_behind():
    return {os.path.join(t, f) for t in ("/dev/shm", "/tmp") if os.path.isdir(t) for f in os.listdir(t) if f.startswith("rfx_packed_")}


def test_packed_cache_route_and_its_fallbacks_host_side(harness, packed_dir):
    """What tests/test_cli_gpu.py::test_subject_is_parsed_once_and_filtered_from_the_packed_cache asserts on the device, over
    the host stand-ins: `--packed` writes what `--sam` writes and touches text only for the names with a hit; a cache packed
    for another MinQ and a cache its producer did not finish send the run down the text route, which says so."""
    d = packed_dir
    n_records = sum(1 for ln in open(f"{d}/in.sam", "rb") if ln.count(b"\t") >= 10)
    before = _left_behind()
    tail = ["25", "15", "1", "4"]
    r = _run(harness, d, ["--sam", "text.chr", "hl", "in.sam", "text"] + tail)
    assert r.returncode == 0, r.stderr
    r20 = _run(harness, d, ["--sam", "text20.chr", "hl", "in.sam", "text20", "25", "20", "1", "4"])
    assert r20.returncode == 0, r20.stderr
    want, want20 = _outputs(d, "text"), _outputs(d, "text20")
    assert want[0].count(b"\n") >= 80 and want[1].count(b"\n") >= 80

    r = _run(harness, d, ["--packed", "cache.bin", "packed.chr", "hl", "in.sam", "packed"] + tail)
    assert r.returncode == 0 and r.stderr == b"", r.stderr
    assert _outputs(d, "packed") == want
    line = [ln for ln in r.stdout.split(b"\n") if ln.startswith(b"packed cache:")]
    assert len(line) == 1
    words = line[0].split()
    scanned, gathered = int(words[2]), int(words[-3])
    assert words[3:5] == [b"records", b"scanned,"] and words[-2:] == [b"lines", b"gathered"]
    assert scanned == n_records and 0 < gathered < n_records
    # the inner --sam run's own lines come after the cache's
    assert r.stdout.index(b"packed cache:") < r.stdout.index(b"Call is --sam") < r.stdout.index(b"Done Hash Files")
    assert r.stdout.count(b"Done Hash Files") == 1 and r.stdout.endswith(b"\nDone running RUFUS.Filter.cpp\n")

    r = _run(harness, d, ["--packed", "cache.bin", "otherq.chr", "hl", "in.sam", "otherq", "25", "20", "1", "4"])
    assert r.returncode == 0, r.stderr
    assert b"not a usable packed-read cache" in r.stderr and b"packed cache:" not in r.stdout
    assert _outputs(d, "otherq") == want20

    blob = bytearray(open(f"{d}/cache.bin", "rb").read())
    blob[16:24] = bytes(8)                                   # the "done" word: its producer did not finish
    open(f"{d}/undone.bin", "wb").write(blob)
    r = _run(harness, d, ["--packed", "undone.bin", "undone.chr", "hl", "in.sam", "undone"] + tail)
    assert r.returncode == 0, r.stderr
    assert b"scanning the text" in r.stderr and b"packed cache:" not in r.stdout
    assert _outputs(d, "undone") == want
    assert _left_behind() <= before


CALL_TEXT = b"Call is PreBuiltMutHash Mutant.Mate1.fq Mutant.Mate2.fq firstpassfile hashsize MinQ HashCountThreshold threads \n"
CALL_TEXT_SE = b"Call is PreBuiltMutHash Mutant.fq|stdin firstpassfile hashsize MinQ HashCountThreshold threads\n"
CALL_SAM = b"Call is --sam CHRFILE PreBuiltMutHash SAM|stdin firstpassfile hashsize MinQ HashCountThreshold threads\n"
CALL_BAM = (b"Call is --bam CHRFILE PreBuiltMutHash X.bam firstpassfile hashsize MinQ HashCountThreshold threads [--bam-exclude N] "
            b"[--region REG]\n")
CALL_PACKED = b"Call is --packed CACHE CHRFILE PreBuiltMutHash SPOOL firstpassfile hashsize MinQ HashCountThreshold threads\n"
NO_HL, NO_IN = b"Error, ParentHashFile could not be opened", b"Error, MutFile could not be opened"
NO_OUT = b"ERROR, Output file could not be opened -nodir/o\n"
DONE_HASH = b"\nDone Hash Files\n\t Mutations Hash size is "
T = ["25", "15", "1", "2"]
# name: (executable, arguments, exit status, stdout, stderr) -- status and both streams as the executables gave them before
# the routes were given one front and one finish (recorded from that build; run in packed_dir)
REFUSALS = {
    "text_few": ("paired", ["hl"], 0, CALL_TEXT + b"ERROR: expected 8 arguments\n", b""),
    "sam_few": ("paired", ["--sam", "o.chr"], 0, CALL_SAM + b"ERROR: expected 9 arguments\n", b""),
    "bam_few": ("paired", ["--bam", "o.chr"], 0, CALL_BAM + b"ERROR: expected 9 arguments\n", b""),
    "packed_few": ("paired", ["--packed", "cache.bin"], 0, CALL_PACKED + b"ERROR: expected 10 arguments\n", b""),
    "single_text_few": ("single", [], 0, CALL_TEXT_SE + b"ERROR: expected 7 arguments\n", b""),
    "single_sam_few": ("single", ["--sam"], 0, CALL_SAM + b"ERROR: expected 9 arguments\n", b""),
    "single_bam_few": ("single", ["--bam"], 0, CALL_BAM + b"ERROR: expected 9 arguments\n", b""),
    "text_no_hashlist": ("paired", ["nohl", "m1.fq", "m2.fq", "o"] + T, 0, CALL_TEXT + NO_HL, b""),
    "sam_no_hashlist": ("paired", ["--sam", "o.chr", "nohl", "in.sam", "o"] + T, 0, CALL_SAM + NO_HL, b""),
    "bam_no_hashlist": ("paired", ["--bam", "o.chr", "nohl", "in.sam", "o"] + T, 0, CALL_BAM + NO_HL, b""),
    "packed_no_hashlist": ("paired", ["--packed", "cache.bin", "o.chr", "nohl", "in.sam", "o"] + T, 0, CALL_PACKED + NO_HL, b""),
    "text_no_mate1": ("paired", ["hl", "nom1.fq", "m2.fq", "o"] + T, 0, CALL_TEXT + NO_IN, b""),
    "text_no_mate2": ("paired", ["hl", "m1.fq", "nom2.fq", "o"] + T, 0, CALL_TEXT + NO_IN, b""),
    "sam_no_input": ("paired", ["--sam", "o.chr", "hl", "no.sam", "o"] + T, 0, CALL_SAM + NO_IN, b""),
    "bam_no_input": ("paired", ["--bam", "o.chr", "hl", "no.bam", "o"] + T, 0, CALL_BAM + NO_IN, b""),
    "packed_no_spool": ("paired", ["--packed", "cache.bin", "o.chr", "hl", "no.sam", "o"] + T, 0, CALL_PACKED + NO_IN, b""),
    "single_sam_no_input": ("single", ["--sam", "o.chr", "hl", "no.sam", "o"] + T, 0, CALL_SAM + NO_IN, b""),
    "text_no_stub": ("paired", ["hl", "m1.fq", "m2.fq", "nodir/o"] + T, 0, CALL_TEXT + NO_OUT, b""),
    "sam_no_stub": ("paired", ["--sam", "o.chr", "hl", "in.sam", "nodir/o"] + T, 0, CALL_SAM + NO_OUT, b""),
    "sam_no_chr": ("paired", ["--sam", "nodir/o.chr", "hl", "in.sam", "o"] + T, 0, CALL_SAM + b"ERROR, Output file could not be opened -o\n", b""),
    "single_sam_no_stub": ("single", ["--sam", "o.chr", "hl", "in.sam", "nodir/o"] + T, 0, CALL_SAM + NO_OUT, b""),
    "single_text_no_stub": ("single", ["hl", "m1.fq", "nodir/o"] + T, 0, CALL_TEXT_SE + NO_OUT, b""),
    "text_k0": ("paired", ["hl", "m1.fq", "m2.fq", "o", "0", "15", "1", "2"], 1, CALL_TEXT, b"rufus_amd RUFUS.Filter: hash size must be 1..32\n"),
    "text_k33": ("paired", ["hl", "m1.fq", "m2.fq", "o", "33", "15", "1", "2"], 1, CALL_TEXT, b"rufus_amd RUFUS.Filter: hash size must be 1..32\n"),
    "sam_k0": ("paired", ["--sam", "o.chr", "hl", "in.sam", "o", "0", "15", "1", "2"], 1, CALL_SAM, b"rufus_amd RUFUS.Filter: hash size must be 1..32\n"),
    "sam_k33": ("paired", ["--sam", "o.chr", "hl", "in.sam", "o", "33", "15", "1", "2"], 1, CALL_SAM, b"rufus_amd RUFUS.Filter: hash size must be 1..32\n"),
    "packed_k0": ("paired", ["--packed", "cache.bin", "o.chr", "hl", "in.sam", "o", "0", "15", "1", "2"], 1, CALL_PACKED,
                  b"rufus_amd RUFUS.Filter: hash size must be 1..32\n"),
    "packed_k33": ("paired", ["--packed", "cache.bin", "o.chr", "hl", "in.sam", "o", "33", "15", "1", "2"], 1, CALL_PACKED,
                   b"rufus_amd RUFUS.Filter: hash size must be 1..32\n"),
    "single_text_k0": ("single", ["hl", "m1.fq", "o", "0", "15", "1", "2"], 1, CALL_TEXT_SE, b"rufus_amd RUFUS.Filter: hash size must be 1..32\n"),
    "single_sam_k33": ("single", ["--sam", "o.chr", "hl", "in.sam", "o", "33", "15", "1", "2"], 1, CALL_SAM,
                       b"rufus_amd RUFUS.Filter.single: hash size must be 1..32\n"),
    "bam_not_bgzf": ("paired", ["--bam", "o.chr", "hl", "in.sam", "o"] + T, 1, CALL_BAM, b"rufus_amd RUFUS.Filter: --bam: 'in.sam' is not BGZF\n"),
    "bam_unknown_argument": ("paired", ["--bam", "o.chr", "hl", "in.sam", "o"] + T + ["--what"], 1, CALL_BAM,
                             b"rufus_amd RUFUS.Filter: --bam: unknown argument --what\n"),
    "single_packed": ("single", ["--packed", "cache.bin", "o.chr", "hl", "in.sam", "o"] + T, 1, b"",
                      b"rufus_amd RUFUS.Filter.single: --packed is for paired subjects only (RUFUS.Filter --packed): use --bam or --sam\n"),
    "packed_region": ("paired", ["--packed", "cache.bin", "o.chr", "hl", "in.sam", "o"] + T + ["--region", "chr1"], 1, CALL_PACKED,
                      b"rufus_amd RUFUS.Filter: --region does not go with --packed: the cache does not record a region (use --bam)\n"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_are_what_they_were(harness, single_harness, packed_dir, name):
    exe, args, status, stdout, stderr = REFUSALS[name]
    r = _run(harness if exe == "paired" else single_harness, packed_dir, args)
    assert (r.returncode, r.stdout, r.stderr) == (status, stdout, stderr)


@pytest.mark.parametrize("sync_open", [False, True])
def test_empty_sequence_line_is_refused_with_status_1(harness, packed_dir, tmp_path, sync_open):
    """The text route refuses from a worker thread, beside the thread that opens the device: it waits for that thread and
    leaves with status 1 and its sentence, with the device opened beside the readers and (RFX_SYNC_OPEN=1) before them."""
    d = str(tmp_path)
    rec = b"@r%d\n%s\n+\n%s\n"
    open(f"{d}/m1.fq", "wb").write(b"@r0\n\n+\n\n" + b"".join(rec % (i, b"ACGTTGCA" * 8, b"I" * 64) for i in range(1, 4)))
    open(f"{d}/m2.fq", "wb").write(b"".join(rec % (i, b"TTGCAACG" * 8, b"I" * 64) for i in range(4)))
    r = _run(harness, d, [f"{packed_dir}/hl", "m1.fq", "m2.fq", "o"] + T, **({"RFX_SYNC_OPEN": "1"} if sync_open else {}))
    assert r.returncode == 1
    assert r.stderr == b"rufus_amd RUFUS.Filter: empty sequence line (undefined behaviour in the reference) -- rejected\n"
    assert r.stdout.startswith(CALL_TEXT + DONE_HASH)
    # the same with a device that takes 300 ms to start (the stand-in's rfx_open): die() waits for the opener thread
    # (rfx_cli.hpp Opener), so the harness does not see an exit beside a running rfx_open
    slow = _run(harness, d, [f"{packed_dir}/hl", "m1.fq", "m2.fq", "o"] + T, RFX_TEST_OPEN_MS="300",
                **({"RFX_SYNC_OPEN": "1"} if sync_open else {}))
    assert (slow.returncode, slow.stderr) == (r.returncode, r.stderr)
