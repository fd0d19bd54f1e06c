"""Host references of the assembly-side kernels (K6 overlap scoring, K7 mutant k-mer coverage), restated from the
reference's text: Align3 of src/OverlapSam.cpp / src/Overlap.cpp / src/OverlapRegion.cpp and the window loop of
src/AnnotateOverlap.cpp:88-134.  Plain Python and numpy, no device, no library call."""
import functools

import numpy as np

_N = ord("N")


def align3_one(a: bytes, b: bytes, min_pct: float, min_ovl: int, strict3: bool, init: int):
    """Per-candidate body of Align3 (src/OverlapSam.cpp:47-229 / src/Overlap.cpp:176-340), float32 as the
    reference: returns (p1 score, p1 overlap, perfect, full score, full overlap)."""
    f = np.float32
    al, bl = len(a), len(b)
    asm = not (bl > al)
    window, longest = (bl, al) if asm else (al, bl)
    mm = int(f(window) - f(window) * f(min_pct))
    best, ovl, perfect = init, 0, False
    ac = bc = 0
    for i in range(longest - window + 1):
        score = f(0)
        for k in range(window):
            if a[k + ac] == b[k + bc] and b[k + bc] != ord("N"):
                score += f(1)
            if f(k) - score > mm:
                score = f(-1)
                break
        if asm:
            ac += 1
        else:
            bc += 1
        if window and f(score / f(window)) >= f(min_pct):
            if best < score:
                best, ovl = int(score), (-i if asm else i)
            if score == window:
                perfect = True
                break
    p1 = (best, ovl, perfect)
    if not perfect:
        for phase in (2, 3):
            for i in range(window - 1, min_ovl - 1, -1):
                score, k = f(0), 0
                for k in range(i + 1):
                    x, y = (a[al - i + k - 1], b[k]) if phase == 2 else (b[bl - i + k - 1], a[k])
                    if x == y and y != ord("N"):
                        score += f(1)
                    if f(k) - score > mm:
                        score = f(-1)
                        break
                else:
                    k = i + 1
                pct = f(score / f(k)) if k else f(0)
                ok = pct > f(min_pct) if (phase == 3 and strict3) else pct >= f(min_pct)
                if ok and best < score:
                    best, ovl = int(score), (i - al + 1 if phase == 2 else bl - i - 1)
                    if score == i:
                        break
    return p1[0], p1[1], int(p1[2]), best, ovl


@functools.lru_cache(maxsize=None)
def _offset_scores(a: bytes, b: bytes):
    """Matches (equal, non-'N' bases) of every offset of the three phases, one numpy comparison per offset, in the
    reference's loop order: phase 1 by i = 0 .., phases 2 and 3 by overlap length - 1 = window - 1 down to 0.  They
    depend on the two strings alone, so the settings of one pair share them."""
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    al, bl = len(a), len(b)
    asm = not (bl > al)
    window, longest = (bl, al) if asm else (al, bl)

    def matches(u, v):
        return int(np.count_nonzero((u == v) & (v != _N)))

    p1 = np.array([matches(x[i:i + window], y[:window]) if asm else matches(x[:window], y[i:i + window])
                   for i in range(longest - window + 1)], np.int64)
    down = range(window - 1, -1, -1)
    p2 = np.array([matches(x[al - i - 1:], y[:i + 1]) for i in down], np.int64)
    p3 = np.array([matches(y[bl - i - 1:], x[:i + 1]) for i in down], np.int64)
    return p1, p2, p3


def align3_fast(a: bytes, b: bytes, min_pct: float, min_ovl: int, strict3: bool, init: int, with_phase: bool = False):
    """align3_one's rules on whole offsets: integer scores, the percentage test float32(score) / float32(len) against
    float32(min_pct), the running abort as `len - score - 1 > mm` (mismatches only pile up, so an offset is given up
    somewhere iff it would be at its last base), mm in float32 as the reference computes it.  An aborted offset carries
    -1 / k < 0 in the reference and is accepted under no setting.  Within one loop the first offset with the strictly
    greatest accepted score wins (the reference's `score == i` exit leaves only offsets that are too short to beat it).
    with_phase: also the phase (1, 2, 3; 0 = nothing accepted) that the full result comes from."""
    f = np.float32
    al, bl = len(a), len(b)
    asm = not (bl > al)
    window = bl if asm else al
    mm = int(f(window) - f(window) * f(min_pct))
    s1, s2, s3 = _offset_scores(a, b)
    best, ovl, perfect, phase = init, 0, False, 0

    def accepted(score, length, strict):
        with np.errstate(divide="ignore", invalid="ignore"):
            pct = score.astype(f) / length.astype(f)
        ok = pct > f(min_pct) if strict else pct >= f(min_pct)
        return ok & ~(length - score - 1 > mm)

    if window:
        ok = accepted(s1, np.full(len(s1), window, np.int64), False)
        full = np.flatnonzero(ok & (s1 == window))
        if len(full):                       # the loop ends at the first perfect offset
            ok[full[0] + 1:] = False
            perfect = True
        at = np.flatnonzero(ok)
        if len(at):
            i = int(at[np.argmax(s1[at])])  # (argmax: the first of the greatest)
            if best < s1[i]:
                best, ovl, phase = int(s1[i]), (-i if asm else i), 1
    p1 = (best, ovl, int(perfect))
    if not perfect:
        n = max(window - min_ovl, 0)        # i = window - 1 .. min_ovl
        lens = np.arange(window, window - n, -1, dtype=np.int64)
        for ph, s in ((2, s2[:n]), (3, s3[:n])):
            at = np.flatnonzero(accepted(s, lens, ph == 3 and strict3))
            if len(at):
                t = int(at[np.argmax(s[at])])
                if best < s[t]:
                    i = window - 1 - t
                    best, ovl, phase = int(s[t]), (i - al + 1 if ph == 2 else bl - i - 1), ph
    out = (p1[0], p1[1], p1[2], best, ovl)
    return (out, phase) if with_phase else out


_CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}


def annotate_ref(seqs, quals, keys, k: int) -> np.ndarray:
    """Per-base mutant k-mer coverage of AnnotateOverlap (src/AnnotateOverlap.cpp:88-134), contig after contig, from
    the text: a base is good iff it is not 'N' and qual - 33 >= 3 (no quality character: bad); for p in range(len - 1)
    -- the last base never ends a window -- the k bases ending at p count iff all are good and their code (A0 C1 G2
    T3, first base most significant) is in `keys`; a hit adds 1 to each of its k positions."""
    keys = set(int(x) for x in keys)
    out = []
    for s, q in zip(seqs, quals):
        cov = np.zeros(len(s), np.uint32)
        good = [s[p] != _N and p < len(q) and q[p] - 33 >= 3 for p in range(len(s))]
        for p in range(len(s) - 1):
            lo = p - k + 1
            if lo < 0 or not all(good[lo:p + 1]):
                continue
            code = 0
            for ch in s[lo:p + 1]:
                code = (code << 2) | _CODE[ch]
            if code in keys:
                cov[lo:p + 1] += 1
        out.append(cov)
    return np.concatenate(out) if out else np.zeros(0, np.uint32)
