"""A Python model of the GPU libsvm parser's rule (csrc/kernels/libsvm_rule.h).

Three things, written independently of the header:

* grammar G of a regular line: ``ws* number (ws+ index ':' number)* ws*`` with
  ``ws`` = space, tab, CR; ``index`` = 1..18 digits; ``number`` =
  ``[+-]? digits ('.' digits*)? exp?`` or ``[+-]? '.' digits exp?`` of at most
  15 significant digits and a folded decimal exponent within +-22;
* the value of a number: ``d = m * 10^e`` or ``m / 10^-e`` in one double
  rounding, then ``float32(d)``; *ambiguous* (irregular) when d looks like a
  float32 tie, is non-zero below FLT_MIN, or is above FLT_MAX;
* ``keep(seed, ordinal, rate)``: the splitmix64 finaliser of
  ``seed ^ ordinal * 0x9E3779B97F4A7C15``, top 32 bits below ``rate * 2^32``.

`Model(...)`'s switches turn single rules off: the mutants that
tests/test_libsvm_gpu_reference_cpu.py shows the fixtures can tell apart.
"""
import re
import struct

import numpy as np

WS = b" \t\r"
_NUM = rb"([+-]?)(?:(\d+)(?:\.(\d*))?|\.(\d+))(?:[eE]([+-]?)(\d+))?"
NUM_RE = re.compile(_NUM)
ENTRY_RE = re.compile(rb"(\d{1,18}):")
SPLIT_RE = re.compile(rb"[ \t\r]+")
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
M64 = (1 << 64) - 1

IRREGULAR = "irregular"


def keep(seed, ordinal, rate):
    if rate >= 1.0:
        return True
    z = (seed ^ (ordinal * 0x9E3779B97F4A7C15)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 32) < int(rate * 4294967296.0)


def pieces(data):
    """The '\\n'-separated pieces parse_buffer walks: no piece after a final newline."""
    if not data:
        return []
    out = data.split(b"\n")
    if data.endswith(b"\n"):
        out.pop()
    return out


class Model:
    def __init__(self, tie_flag=True, neg_zero=True, exp_sign=True, end_check=True):
        self.tie_flag, self.neg_zero, self.exp_sign, self.end_check = tie_flag, neg_zero, exp_sign, end_check

    # ---------------------------------------------------------------- numbers
    def number(self, tok):
        """float32 of a number token, or None when it is outside G or ambiguous."""
        m = NUM_RE.fullmatch(tok) if self.end_check else NUM_RE.match(tok)
        if m is None:
            return None
        sign, ip, fp, fp2, esign, edig = m.groups()
        ip = ip or b""
        fp = (fp if fp is not None else fp2) or b""
        digits = (ip + fp).lstrip(b"0")
        if len(digits) > 15:
            return None
        mant = int(digits) if digits else 0
        ex = int(edig) if edig else 0
        if esign == b"-" and self.exp_sign:
            ex = -ex
        e = ex - len(fp)
        if abs(e) > 22:
            return None
        d = float(mant) * float(10 ** e) if e >= 0 else float(mant) / float(10 ** -e)
        bits = struct.unpack("<Q", struct.pack("<d", d))[0]
        if self.tie_flag and (bits & 0x1FFFFFFF) == 0x10000000:
            return None
        if (d != 0.0 and d < FLT_MIN) or d > FLT_MAX:
            return None
        f = np.float32(d)
        if sign == b"-" and (self.neg_zero or f != 0):
            f = -f
        return f

    # ------------------------------------------------------------------ lines
    def line(self, piece):
        """None for a piece that is skipped silently (< 2 bytes), IRREGULAR, or
        (label, [ids], [vals])."""
        if len(piece) < 2:
            return None
        toks = [t for t in SPLIT_RE.split(piece) if t]
        if not toks:
            return IRREGULAR
        label = self.number(toks[0])
        if label is None:
            return IRREGULAR
        ids, vals = [], []
        for t in toks[1:]:
            m = ENTRY_RE.match(t)
            if m is None:
                return IRREGULAR
            v = self.number(t[m.end():])
            if v is None:
                return IRREGULAR
            ids.append(int(m.group(1)))
            vals.append(v)
        return label, ids, vals

    def parse(self, data, rate=1.0, seed=0, first_ordinal=0):
        """dict(irregular, lines, kept (ordinals), labels, offsets, ids, vals).  A chunk with
        an irregular line, kept or not, is irregular as a whole: the GPU decides before it samples."""
        labels, offsets, ids, vals, kept = [], [0], [], [], []
        irregular = False
        ps = pieces(data)
        for k, p in enumerate(ps):
            r = self.line(p)
            if r is None:
                continue
            if r == IRREGULAR:
                irregular = True
                continue
            if not keep(seed, first_ordinal + k, rate):
                continue
            kept.append(first_ordinal + k)
            labels.append(r[0])
            ids.extend(r[1])
            vals.extend(r[2])
            offsets.append(len(ids))
        return dict(irregular=irregular, lines=len(ps), kept=kept, labels=np.array(labels, np.float32),
                    offsets=np.array(offsets, np.int64), ids=np.array(ids, np.int64), vals=np.array(vals, np.float32))


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)
