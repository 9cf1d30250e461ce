"""Which batches the MLP runners of `models/mlp.py` launch next: integer
bookkeeping only (no torch, no native module), so it is tested on the CPU
(tests/test_mlp_runner_plan_cpu.py)."""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

Chunk = Tuple[int, int]     # (first batch of the epoch, steps)


def chunks(cursor: int, steps: int, g: int, nb: int, wrap: bool) -> List[Chunk]:
    """The next `steps` steps from global batch index `cursor` as chunks of at
    most `g` steps over an epoch of `nb` batches.  wrap: a chunk may run across
    the epoch boundary (`MLPStepRunner` copies it in two pieces); else it stops
    there (`StagePlanner`: a stage holds consecutive host records)."""
    out = []
    while steps > 0:
        b0 = cursor % nb
        n = min(g, steps) if wrap else min(g, steps, nb - b0)
        out.append((b0, n))
        cursor += n
        steps -= n
    return out


def _covers(s: Optional[Chunk], r: Chunk) -> bool:
    return s is not None and s[0] <= r[0] and r[0] + r[1] <= s[0] + s[1]


class StagePlanner:
    """Staging of `PersistentMLPRunner`: two device stages, each holding one chunk
    of consecutive batches; `launch(par, off, nsteps, host_off, next_steps)`
    computes `nsteps` steps from stage `par` at step offset `off` and copies
    `next_steps` records from byte `host_off` of the epoch into stage `par ^ 1`.

    Range-based: steps that lie inside a staged chunk run from it at an offset,
    and a chunk already resident in the other stage is not copied again.  The
    chunk copied inside a launch is the next planned one or, for the last launch
    of a `run()`, a speculative chunk as long as that `run()` (`lookahead`
    overrides the length), so a short run never streams more than it computes.
    A miss (cold start, plan change) costs a copy-only launch, counted in
    `copy_only_launches`."""

    def __init__(self, num_batches: int, rec: int, g: int, launch: Callable[[int, int, int, int, int], None]):
        self.nb, self.rec, self.g, self.launch = int(num_batches), int(rec), int(g), launch
        self.cursor = 0                                          # next batch index (global)
        self.staged: List[Optional[Chunk]] = [None, None]        # chunk resident per stage
        self.copy_only_launches = 0
        self.last_prefetch_steps = 0

    def _launch(self, par: int, off: int, nsteps: int, nxt: Chunk):
        self.launch(par, off, nsteps, nxt[0] * self.rec, nxt[1])
        if nxt[1] > 0:
            self.staged[par ^ 1] = nxt
        self.last_prefetch_steps = nxt[1]

    def _ensure(self, c: Chunk) -> Tuple[int, int]:
        """(stage, step offset) holding chunk `c`, after a copy-only launch on a miss."""
        for par in (0, 1):
            s = self.staged[par]
            if s is not None and s[0] <= c[0] and c[0] + c[1] <= s[0] + s[1]:
                return par, c[0] - s[0]
        dst = 1 if self.staged[0] is not None and self.staged[1] is None else 0
        self._launch(dst ^ 1, 0, 0, c)     # the stage it "runs" from is untouched
        self.copy_only_launches += 1
        return dst, 0

    def prepare(self, steps: int):
        """Stage the first chunk of the next `run(steps)`."""
        self._ensure(chunks(self.cursor, steps, self.g, self.nb, False)[0])

    def invalidate(self):
        """Forget the staged chunks (the host epoch was re-packed)."""
        self.staged = [None, None]

    def run(self, steps: int, lookahead: Optional[int] = None, launched: Optional[Callable[[int], None]] = None):
        """Launch the next `steps` steps; `launched(n)` follows each compute launch of n steps."""
        g, nb = self.g, self.nb
        la = min(g, steps if lookahead is None else int(lookahead))
        ch = chunks(self.cursor, steps, g, nb, False)
        # behind the last chunk: the speculative one
        ch.append(chunks(self.cursor + steps, la, g, nb, False)[0] if la > 0 else (0, 0))
        for k in range(len(ch) - 1):
            c, nxt = ch[k], ch[k + 1]
            par, off = self._ensure(c)
            if nxt[1] > 0 and _covers(self.staged[par ^ 1], nxt):
                nxt = (nxt[0], 0)           # already resident in the other stage: nothing to stream
            self._launch(par, off, c[1], nxt)
            if launched is not None:
                launched(c[1])
            self.cursor += c[1]
