"""The GPU libsvm parser's rule against libc, on the CPU.

The GPU parser accepts a strict grammar and computes a number as one double
rounding of mantissa * 10^exponent followed by a cast to float32; everything it
cannot prove equal to strtof it hands back to the C++ parser.  This file checks
that rule -- through its Python model, tests/libsvm_gpu_reference.py -- against
`libsvm_parse_bytes` (strtof / strtoll): on random regular numbers, on decimal
strings generated around float32 midpoints (where the double rounding can go
wrong: the tie flag must catch every such string), and that the fixtures can
tell four broken models from the right one.  It also checks the hashed host
parser (`libsvm_parse_bytes_hashed`, the GPU parser's fallback and its
rate < 1 sample) against the model's `keep()`.
"""
import numpy as np
import pytest

import libsvm_gpu_reference as R


@pytest.fixture(scope="module")
def C(native):
    return native


def _cpu(C, data):
    y, rp, ids, vals = C.libsvm_parse_bytes(data, 1.0, 0)
    return np.asarray(y, np.float32), np.asarray(rp, np.int64), np.asarray(ids, np.int64), np.asarray(vals, np.float32)


def _random_numbers(n, seed):
    """n G numbers: 1..15 significant digits, the point anywhere (also first and
    last), leading zeros, signs, exponents so that the folded exponent covers
    [-22, 22]; one in 50 a signed zero."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        sign = ("", "+", "-")[rng.integers(3)]
        if i % 50 == 0:
            out.append(sign + ("0", "0.0", ".0", "0.", "00", "0e0", "0.00e+2", "0E-3")[rng.integers(8)])
            continue
        nd = int(rng.integers(1, 16))
        digits = str(rng.integers(1, 10)) + "".join(str(d) for d in rng.integers(0, 10, nd - 1))
        fl = int(rng.integers(0, nd + 1))                  # fraction digits
        e10 = int(rng.integers(-22, 23))                   # folded exponent
        ip, fp = digits[:nd - fl], digits[nd - fl:]
        if rng.integers(4) == 0:
            ip = "0" * int(rng.integers(1, 3)) + ip
        body = (ip + "." + fp) if (fp or rng.integers(3) == 0) else ip
        if body.startswith(".") and not fp:
            body = "0" + body
        ex = e10 + fl
        if ex != 0 or rng.integers(3) == 0:
            body += "eE"[rng.integers(2)] + ("-" if ex < 0 else ("+" if rng.integers(2) else "")) + \
                ("0" if rng.integers(5) == 0 else "") + str(abs(ex))
        out.append(sign + body)
    return out


def _lines_of(numbers, per_line=4):
    """`label id:v id:v id:v` lines over the numbers (the label is a number of the set too)."""
    lines = []
    for s in range(0, len(numbers) - per_line + 1, per_line):
        g = numbers[s:s + per_line]
        lines.append(g[0] + " " + " ".join(f"{7 * k + 1}:{v}" for k, v in enumerate(g[1:])))
    return lines


def _compare(C, lines, model):
    """(accepted lines, mismatching lines) of `model` against the C++ parser, line by line;
    every line is one the C++ parser takes."""
    data = ("\n".join(lines) + "\n").encode()
    y, rp, ids, vals = _cpu(C, data)
    assert len(y) == len(lines)
    yb, vb = R.bits32(y), R.bits32(vals)
    accepted = wrong = 0
    for k, ln in enumerate(lines):
        r = model.line(ln.encode())
        if r == R.IRREGULAR:
            continue
        accepted += 1
        s, e = rp[k], rp[k + 1]
        ok = (R.bits32([r[0]])[0] == yb[k] and list(ids[s:e]) == r[1]
              and np.array_equal(R.bits32(r[2]), vb[s:e]))
        wrong += not ok
    return accepted, wrong


@pytest.fixture(scope="module")
def regular_lines():
    return _lines_of(_random_numbers(200_000, seed=11))


def _near_tie_strings(count, seed):
    """Decimal strings around float32 midpoints: each midpoint printed to 9, 12 and 15
    significant digits with the last digit moved by -1, 0, +1 (as `<mantissa>e<exp>`)."""
    rng = np.random.default_rng(seed)
    out = []
    lo = np.float32(1e-6).view(np.uint32)
    hi = np.float32(1e6).view(np.uint32)
    bits = rng.integers(int(lo), int(hi), count, dtype=np.int64).astype(np.uint32)
    for b in bits:
        f0 = float(np.uint32(b).view(np.float32))
        f1 = float(np.uint32(b + 1).view(np.float32))
        mid = (f0 + f1) / 2                                 # exact in a double
        for k in (9, 12, 15):
            mant, ex = f"{mid:.{k - 1}e}".split("e")
            m = int(mant.replace(".", ""))
            for d in (-1, 0, 1):
                out.append(f"{m + d}e{int(ex) - (k - 1)}")
    return out


@pytest.fixture(scope="module")
def tie_lines():
    return _lines_of(_near_tie_strings(12_000, seed=5), per_line=2)


def test_random_regular_numbers_equal_strtof_bit_for_bit(C, regular_lines):
    accepted, wrong = _compare(C, regular_lines, R.Model())
    print(f"regular lines: {len(regular_lines)}, accepted {accepted}, mismatching {wrong}")
    assert wrong == 0
    # what the model hands back are the odd integers of [2^24, 2^25) and their like: true float ties
    assert accepted >= 0.95 * len(regular_lines)


def test_near_tie_strings_every_accepted_value_equals_strtof(C, tie_lines):
    accepted, wrong = _compare(C, tie_lines, R.Model())
    print(f"near-tie lines: {len(tie_lines)}, accepted {accepted}, mismatching {wrong}")
    assert wrong == 0
    assert accepted >= 0.5 * len(tie_lines)


def test_fixtures_tell_the_mutants_apart(C, regular_lines, tie_lines):
    _, no_tie = _compare(C, tie_lines, R.Model(tie_flag=False))
    print(f"tie flag removed: {no_tie} mismatching lines of {len(tie_lines)}")
    assert no_tie >= 1
    _, no_negzero = _compare(C, regular_lines, R.Model(neg_zero=False))
    assert no_negzero >= 1
    _, no_expsign = _compare(C, regular_lines, R.Model(exp_sign=False))
    assert no_expsign >= 1
    # "3:0.5abc": strtof stops at 'a', strtoll then fails on "abc": the C++ parser drops the line
    data = b"1 3:0.5abc\n0 4:2\n"
    y, rp, ids, vals = _cpu(C, data)
    assert len(y) == 1 and list(ids) == [4]
    assert R.Model().line(b"1 3:0.5abc") == R.IRREGULAR
    loose = R.Model(end_check=False).line(b"1 3:0.5abc")
    assert loose != R.IRREGULAR and loose[1] == [3]          # the mutant keeps a line the C++ parser drops


@pytest.mark.parametrize("tok", [
    "inf", "nan", "-inf", "0x1p3", "0x10", "1e", "1e+", ".", "+", "-", "1.2.3", "1e5.0", "1,5",
    "1234567890123456", "1e23", "1e-23", "0.1e24", "16777217", "1e40", "1e-40", "3.5e38", "--1", "1 e5"])
def test_numbers_outside_the_grammar_or_ambiguous(tok):
    assert R.Model().number(tok.encode()) is None


@pytest.mark.parametrize("piece", [
    b"1 3: 0.5", b"1 3:4:5", b"1 3:", b"1 :5", b"1 +3:1", b"1 -3:1", b"1 1234567890123456789:1", b"  ", b"\r\r",
    b"1 3:1\x00", b"1 3:1\x80", b"1 3:1\v", b"3:1 4:1", b"1 2", b"1\f2:3", b"1 2:3abc"])
def test_irregular_lines(piece):
    assert R.Model().line(piece) == R.IRREGULAR


def test_regular_edge_lines():
    m = R.Model()
    assert m.line(b"") is None and m.line(b"1") is None and m.line(b"\r") is None
    lab, ids, vals = m.line(b" \t-1 \t 0:5. \t999999999999999999:.5  7:1E+3 8:1e-5 9:-0 \r")
    assert lab == -1 and ids == [0, 999999999999999999, 7, 8, 9]
    assert list(R.bits32(vals)) == list(R.bits32([5.0, 0.5, 1000.0, 1e-5, -0.0]))
    assert m.line(b"-1") == (np.float32(-1), [], [])


def test_hashed_parser_keeps_exactly_the_lines_keep_names(C):
    rng = np.random.default_rng(3)
    lines = []
    for k in range(6000):
        if k % 97 == 0:
            lines.append("")                       # pieces shorter than 2 bytes count in the ordinal
        elif k % 89 == 0:
            lines.append("7")
        elif k % 101 == 0:
            lines.append("1 bad")                  # a bad line: counted, dropped
        else:
            lines.append(f"{k % 2} " + " ".join(f"{int(i)}:{k}.5" for i in rng.integers(0, 1000, int(rng.integers(0, 5)))))
    data = ("\n".join(lines) + "\n").encode()
    seed, first, rate = 12345, 17, 0.3
    y, rp, ids, vals, pieces, bad = C.libsvm_parse_bytes_hashed(data, rate, seed, first)
    assert pieces == len(lines)
    want = [ln for k, ln in enumerate(lines) if len(ln) >= 2 and ln != "1 bad" and R.keep(seed, first + k, rate)]
    assert 0.25 * len(lines) < len(want) < 0.35 * len(lines)
    assert bad == sum(1 for k, ln in enumerate(lines) if ln == "1 bad" and R.keep(seed, first + k, rate))
    ry, rrp, rids, rvals = _cpu(C, ("\n".join(want) + "\n").encode())
    assert np.array_equal(R.bits32(y), R.bits32(ry)) and np.array_equal(rp, rrp)
    assert np.array_equal(ids, rids) and np.array_equal(R.bits32(vals), R.bits32(rvals))
    # another first ordinal keeps other lines; rate 1 is libsvm_parse_bytes
    y2 = C.libsvm_parse_bytes_hashed(data, rate, seed, first + 1)[0]
    assert len(y2) != len(y) or not np.array_equal(y2, y)
    full = C.libsvm_parse_bytes_hashed(data, 1.0, seed, first)
    fy, frp, fids, fvals = _cpu(C, data)
    assert np.array_equal(R.bits32(full[0]), R.bits32(fy)) and np.array_equal(full[1], frp)
    assert np.array_equal(full[2], fids) and np.array_equal(R.bits32(full[3]), R.bits32(fvals))
    assert full[4] == len(lines) and full[5] == sum(1 for ln in lines if ln == "1 bad")
    for bad_rate in (0.0, 1.5, -0.1):
        with pytest.raises(Exception):
            C.libsvm_parse_bytes_hashed(data, bad_rate, seed, first)


def test_keep_is_a_fair_deterministic_sample():
    got = [R.keep(9, k, 0.3) for k in range(100_000)]
    assert abs(sum(got) / len(got) - 0.3) < 0.01
    assert got == [R.keep(9, k, 0.3) for k in range(100_000)]
    assert all(R.keep(9, k, 1.0) for k in range(100))
