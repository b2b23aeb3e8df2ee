"""The device text parser's fast grammar and value rule ("Text loading"; csrc/text_number.hpp, kernels_text.inc)
restated in Python, and the text cases both parser test files use.  Python's float arithmetic is IEEE binary64 with round to
nearest even and int -> float is correctly rounded, so the restatement rounds where the C++ does."""
import struct

import numpy as np

REASONS = ["none", "too_long", "grammar", "number", "unsorted", "range", "near_tie"]   # by code; the smallest on a line counts
CODE = {name: code for code, name in enumerate(REASONS)}
MAX_SIG_DIGITS, MAX_NET_EXP, MAX_EXP_DIGITS, MAX_FID_DIGITS = 19, 44, 4, 9
POW10 = [float(10 ** k) for k in range(23)]                                             # exact: 10^22 < 2^53 * 2^22
DIGITS = b"0123456789"


def fast_number(tok: bytes):
    """(reason name, f64 value or None) of one token."""
    i, n, neg = 0, len(tok), False
    if i < n and tok[i:i + 1] in (b"-", b"+"):
        neg, i = tok[i:i + 1] == b"-", i + 1
    m = sig = frac = digits = 0
    dot = False
    while i < n:
        c = tok[i:i + 1]
        if c == b".":
            if dot:
                return "number", None
            dot = True
        elif c in DIGITS and c:
            digits += 1
            frac += 1 if dot else 0
            if sig > 0 or c != b"0":
                sig += 1
                if sig > MAX_SIG_DIGITS:
                    return "number", None
                m = m * 10 + int(c)
        else:
            break
        i += 1
    if digits == 0:
        return "number", None
    ex = 0
    if i < n:
        if tok[i:i + 1] not in (b"e", b"E"):
            return "number", None
        i += 1
        eneg = False
        if i < n and tok[i:i + 1] in (b"-", b"+"):
            eneg, i = tok[i:i + 1] == b"-", i + 1
        e0 = i
        while i < n and tok[i:i + 1] in DIGITS:
            ex, i = ex * 10 + int(tok[i:i + 1]), i + 1
        if i == e0 or i - e0 > MAX_EXP_DIGITS or i != n:
            return "number", None
        ex = -ex if eneg else ex
    E = ex - frac
    a = abs(E)
    if a > MAX_NET_EXP:
        return "number", None
    d = float(m)
    p1 = POW10[min(a, 22)]
    d = d / p1 if E < 0 else d * p1
    if a > 22:
        p2 = POW10[a - 22]
        d = d / p2 if E < 0 else d * p2
    if m != 0 and (d < 2.0 ** -126 or d > 3.4e38):
        return "range", None
    low = (struct.unpack("<Q", struct.pack("<d", d))[0] & 0x1FFFFFFF) - 0x10000000
    if -4 <= low <= 4:
        return "near_tie", None
    return "none", (-d if neg else d)


def line_reason(line: bytes, stage_limit: int) -> str:
    """Why the device hands this line (without its newline) back to the host parser, or "none"."""
    if len(line) > stage_limit:
        return "too_long"
    toks = line.split(b"#", 1)[0].split()
    codes = [CODE["grammar"]] if len(toks) < 3 else []
    prev = -1
    for t, tok in enumerate(toks):
        if t == 0:
            codes.append(CODE[fast_number(tok)[0]])
        elif t == 1:
            codes.append(CODE["grammar"] if not (len(tok) > 4 and tok.startswith(b"qid:")) or tok[4:8] == b"qid:" else 0)
        else:
            fid, colon, val = tok.partition(b":")
            if not colon or not (1 <= len(fid) <= MAX_FID_DIGITS) or not fid.isdigit() or any(c not in DIGITS for c in fid):
                codes.append(CODE["grammar"])
                prev = -1
                continue
            codes.append(CODE[fast_number(val)[0]])
            if int(fid) <= prev:
                codes.append(CODE["unsorted"])
            prev = int(fid)
    codes = [c for c in codes if c]
    return REASONS[min(codes)] if codes else "none"


def text_reasons(text: bytes, stage_limit: int):
    """line_reason of every line of a text (a last line without a newline is a line, a trailing newline makes none)."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [line_reason(ln, stage_limit) for ln in lines]


def exact_f32_bytes(tok: str) -> bytes:
    """The f32 nearest the decimal `tok` (ties to even), from exact rational arithmetic: what a correctly rounded strtof gives."""
    from fractions import Fraction
    neg = tok.startswith("-")
    x = Fraction(tok.lstrip("+-"))
    c = np.float32(float(x))
    cands = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    cands = [v for v in cands if np.isfinite(v) and v >= 0]
    best = min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(-best if neg else best).tobytes()


def f32_midpoint_decimal(rng, digits):
    """The decimal expansion, cut at `digits` significant digits, of the exact midpoint of two neighbouring positive normal f32."""
    from fractions import Fraction
    bits = int(rng.integers(0x00800000, 0x7F000000))
    lo, hi = (np.array([b], dtype=np.uint32).view(np.float32)[0] for b in (bits, bits + 1))
    mid = (Fraction(float(lo)) + Fraction(float(hi))) / 2
    e = 0
    while mid >= 10:
        mid, e = mid / 10, e + 1
    while mid < 1:
        mid, e = mid * 10, e - 1
    return "%de%d" % (int(mid * 10 ** (digits - 1)), e - (digits - 1))


def random_tokens(rng, count):
    """Tokens of the classes the value rule was checked on: %g, integers up to 2^50, fixed and exponent forms, 17-digit repr,
    decimal expansions of exact f32 midpoints cut at 8-17 digits."""
    out = []
    for i in range(count):
        k = i % 7
        v = float(np.ldexp(rng.uniform(0.5, 1.0), int(rng.integers(-40, 40)))) * (1 if rng.random() < 0.8 else -1)
        if k == 0:
            out.append("%g" % v)
        elif k == 1:
            out.append(str(int(rng.integers(0, 2 ** 50)) >> int(rng.integers(0, 50))))
        elif k == 2:
            out.append("%.*f" % (int(rng.integers(0, 12)), float(rng.uniform(-1000, 1000))))
        elif k == 3:
            out.append("%.*e" % (int(rng.integers(0, 17)), v))
        elif k == 4:
            out.append(repr(v))
        elif k == 5:
            out.append(repr(float(np.float32(v))))
        else:
            out.append(f32_midpoint_decimal(rng, int(rng.integers(8, 18))))
    return out


def midpoints(rng, digits, count):
    return [f32_midpoint_decimal(rng, digits) for _ in range(count)]


def exact_midpoints(rng, digits, count):
    """Integers of exactly `digits` digits (9 .. 17) that ARE the midpoint of two neighbouring f32: every one is a rounding tie."""
    out = []
    while len(out) < count:
        lo = np.float32(rng.uniform(10.0 ** (digits - 1), 10.0 ** digits * 0.99))
        hi = np.nextafter(lo, np.float32(np.inf))
        mid = (int(lo) + int(hi)) // 2          # both are even integers from 2^25 on
        if len(str(mid)) == digits:
            out.append(str(mid))
    return out


# values the device must hand back or keep, one per line of the "handed back" case (the reason comes from the restatement)
EDGE_VALUES = ["16777217", "12345678901234567890", "0.00012345678901234567890", "1e-40", "1e39", "inf", "nan", "0x1p3", "+1", "-0", ".5", "5.",
               "1e5", "-inf", "1e", ".", "-", "1.2.3", "1e+00005", "1e-45", "3.4e38", "3.5e38", "0e99", "000000000000000000000001.5"]


def mslr_like(rng, lines, feats=136, queries=40):
    """An MSLR-like text: `lines` lines of `feats` features 1..feats, %.6g and integer values, docid comments."""
    rows = []
    vals = rng.uniform(0, 1000, (lines, feats))
    ints = rng.integers(0, 5000, (lines, feats))
    pick = rng.random((lines, feats)) < 0.4
    for i in range(lines):
        body = " ".join("%d:%s" % (j + 1, str(int(ints[i, j])) if pick[i, j] else "%.6g" % vals[i, j]) for j in range(feats))
        rows.append("%d qid:%d %s # doc%d\n" % (int(rng.integers(0, 5)), i * queries // lines, body, i))
    return "".join(rows).encode()
