"""What the MLP runners launch next (models/mlp_plan.py, `MLPStepRunner.plan`):
integer bookkeeping, checked without a GPU or the native module.  The staging
planner is driven through a recording `launch` callable; the test keeps its own
model of what each of the two device stages holds, updated from the recorded
launches only."""
import json
import os
import random
import sys
from types import SimpleNamespace

import pytest

from distributed_tensorflow_example_amd.models.mlp_plan import StagePlanner, chunks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_stage_plan.json")
LOOKAHEADS = (None, 0, 1, 2, 20, 550, 5500)


# ------------------------------------------------------------------ chunker
def _wrapping_chunks_before(cursor, steps, g, nb):
    """`MLPStepRunner._chunks` as it stood before the shared chunker."""
    out, left = [], steps
    while left > 0:
        b0 = cursor % nb
        n = min(g, left)
        out.append((b0, n))
        cursor += n
        left -= n
    return out


@pytest.mark.parametrize("nb", [1, 2, 13, 550])
@pytest.mark.parametrize("g", [1, 5, 550, 1000])
def test_chunks_tile_the_request(nb, g):
    for cursor in (0, 1, nb - 1, nb, 3 * nb + nb // 2, 12345):
        for steps in (0, 1, g - 1, g, g + 1, nb, 2 * nb + 1, 1200):
            for wrap in (False, True):
                ch = chunks(cursor, steps, g, nb, wrap)
                at = cursor
                for b0, n in ch:            # in order, no gap, no overlap
                    assert b0 == at % nb and 1 <= n <= g
                    assert wrap or b0 + n <= nb
                    at += n
                assert at == cursor + max(steps, 0)
            assert chunks(cursor, steps, g, nb, True) == _wrapping_chunks_before(cursor, steps, g, nb)


@pytest.mark.parametrize("cursor, steps, g, nb, wrapping, stopping", [
    (0, 12, 5, 13, [(0, 5), (5, 5), (10, 2)], [(0, 5), (5, 5), (10, 2)]),
    (9, 12, 5, 13, [(9, 5), (1, 5), (6, 2)], [(9, 4), (0, 5), (5, 3)]),
    (0, 3, 1000, 1, [(0, 3)], [(0, 1), (0, 1), (0, 1)]),
    (1, 7, 5, 2, [(1, 5), (0, 2)], [(1, 1), (0, 2), (0, 2), (0, 2)]),
    (540, 20, 550, 550, [(540, 20)], [(540, 10), (0, 10)]),
    (0, 1200, 1000, 550, [(0, 1000), (450, 200)], [(0, 550), (0, 550), (0, 100)]),
    (1100, 1, 550, 550, [(0, 1)], [(0, 1)]),
    (7, 0, 5, 13, [], []),
])
def test_chunks_literals(cursor, steps, g, nb, wrapping, stopping):
    assert chunks(cursor, steps, g, nb, True) == wrapping
    assert chunks(cursor, steps, g, nb, False) == stopping


# ------------------------------------------------------- staging invariants
def _covers(s, b0, n):
    return s is not None and s[0] <= b0 and b0 + n <= s[0] + s[1]


class StageModel:
    """The two device stages as the recorded launches leave them, and every
    property a launch must have given what they hold."""

    def __init__(self, nb, rec):
        self.nb, self.rec = nb, rec
        self.held = [None, None]        # (first batch, batches) resident per stage
        self.cursor = 0                 # next batch to compute (global)
        self.copy_only = 0
        self.log = []

    def launch(self, par, off, nsteps, host_off, next_steps):
        self.log.append((par, off, nsteps, host_off, next_steps))
        assert par in (0, 1) and off >= 0 and nsteps >= 0 and next_steps >= 0
        if nsteps > 0:      # reads batches cursor .. cursor + nsteps - 1 (mod nb) from a stage that holds them
            b0 = self.cursor % self.nb
            s = self.held[par]
            assert s is not None and s[0] + off == b0 and off + nsteps <= s[1] and b0 + nsteps <= self.nb
            self.cursor += nsteps
        else:
            assert off == 0
            self.copy_only += 1
        if next_steps > 0:
            # the copy goes into the other stage (never the one computed from), from the host
            # records of the chunk that is computed next ...
            assert host_off % self.rec == 0
            c0 = host_off // self.rec
            assert c0 == self.cursor % self.nb and c0 + next_steps <= self.nb
            # ... and only when no stage a later launch could run it from holds it already
            assert not _covers(self.held[par ^ 1], c0, next_steps)
            assert nsteps > 0 or not _covers(self.held[par], c0, next_steps)
            self.held[par ^ 1] = (c0, next_steps)
        else:
            assert nsteps > 0, "a launch that neither computes nor copies"

    def invalidate(self):
        self.held = [None, None]        # the host epoch was re-packed: what the stages hold is stale


def _drive(p, m, op, steps, la):
    """One operation on planner `p`, with the checks on what it launched (model `m`)."""
    n0, c0 = len(m.log), p.cursor
    if op == "run":
        p.run(steps, lookahead=la)
        new = m.log[n0:]
        assert p.cursor == c0 + steps == m.cursor
        assert (len(new) > 0) == (steps > 0)
        if new:
            cap = min(p.g, steps if la is None else la)
            assert new[-1][4] <= cap and p.last_prefetch_steps == new[-1][4]
    elif op == "prepare":
        p.prepare(steps)
        b0, n = chunks(c0, steps, p.g, p.nb, False)[0]
        assert p.cursor == c0 and len(m.log) - n0 <= 1
        assert any(_covers(s, b0, n) for s in m.held)
    else:
        p.invalidate()
        m.invalidate()
        assert p.staged == [None, None] and len(m.log) == n0
    assert p.copy_only_launches == m.copy_only == sum(1 for x in m.log if x[2] == 0)
    assert p.staged == m.held


def _random_op(rng):
    op = rng.choice(("run", "run", "run", "prepare", "invalidate"))
    steps = rng.choice((0, 1, 2, 20, rng.randint(0, 1200), rng.randint(0, 60))) if op == "run" else rng.randint(1, 1200)
    return op, steps, rng.choice(LOOKAHEADS)


def test_staging_invariants_over_random_sequences():
    rng = random.Random(20240611)
    nops = 0
    for _ in range(3000):
        nb = rng.choice((1, 2, 13, 550, rng.randint(1, 550)))
        g = rng.choice((1, 5, 550, 1000, rng.randint(1, 1000)))
        rec = rng.choice((16, 78512))
        m = StageModel(nb, rec)
        p = StagePlanner(nb, rec, g, m.launch)
        for _ in range(rng.randint(1, 12)):
            _drive(p, m, *_random_op(rng))
            nops += 1
    assert nops > 15000


def test_resident_chunk_is_not_copied_again():
    m = StageModel(13, 16)
    p = StagePlanner(13, 16, 5, m.launch)
    p.prepare(5)                                    # cold start: chunk (0, 5) into stage 0
    p.run(5, lookahead=5)                           # computes it, prefetches (5, 5) into stage 1
    p.cursor = 0
    m.cursor = 0
    p.run(5, lookahead=5)                           # (0, 5) and (5, 5) are both still resident
    assert m.log == [(1, 0, 0, 0, 5), (0, 0, 5, 5 * 16, 5), (0, 0, 5, 5 * 16, 0)]
    p.run(2, lookahead=0)                           # inside the staged (5, 5), at an offset: no copy at all
    p.run(2, lookahead=None)
    assert m.log[3:] == [(1, 0, 2, 0, 0), (1, 2, 2, 9 * 16, 2)]
    assert p.copy_only_launches == 1 and p.staged == [(9, 2), (5, 5)]


# ------------------------------------------------- the runner before the planner
def _record(driver, ops):
    """The launches of `ops` on `driver` (a StagePlanner, or a runner with the same
    run / prepare / invalidate and counters) and its state afterwards."""
    for op, steps, la in ops:
        if op == "run":
            driver.run(steps, lookahead=la)
        elif op == "prepare":
            driver.prepare(steps)
        else:
            driver.invalidate()
    return {"cursor": driver.cursor, "staged": [None if s is None else list(s) for s in driver.staged],
            "copy_only_launches": driver.copy_only_launches, "last_prefetch_steps": driver.last_prefetch_steps}


def _regenerate(tree):
    """Rewrite the fixture from the `PersistentMLPRunner` of the checkout at `tree` (the commit before
    models/mlp_plan.py existed): its bookkeeping around a recording plan, built without its constructor
    and with the stream lookup stubbed, so no GPU is needed.
    PYTHONPATH=. python tests/test_mlp_runner_plan_cpu.py TREE"""
    for name in [n for n in sys.modules if n.startswith("distributed_tensorflow_example_amd")]:
        del sys.modules[name]
    sys.path.insert(0, tree)
    from distributed_tensorflow_example_amd.models import mlp
    assert mlp.__file__.startswith(tree) and hasattr(mlp.PersistentMLPRunner, "_run_fast"), mlp.__file__
    cfg = {"seed": 7, "nb": 37, "g": 8, "rec": 16, "nops": 300}
    rng = random.Random(cfg["seed"])
    ops = []
    for _ in range(cfg["nops"]):
        op, _, la = _random_op(rng)
        ops.append((op, rng.randint(1 if op == "prepare" else 0, 24), la))
    log = []
    mlp.torch.cuda.current_stream = lambda: None
    r = object.__new__(mlp.PersistentMLPRunner)
    r.epoch, r.g, r.t = SimpleNamespace(num_batches=cfg["nb"], rec=cfg["rec"]), cfg["g"], SimpleNamespace()
    r._plan, r._phase_ts = SimpleNamespace(launch=lambda *a: log.append(list(a))), None
    r.cursor, r.staged, r.copy_only_launches, r.last_prefetch_steps = 0, [None, None], 0, 0
    final = _record(r, ops)
    with open(GOLDEN, "w") as f:
        json.dump({"config": cfg, "ops": [list(o) for o in ops], "launches": log, "final": final}, f,
                  separators=(",", ":"))
        f.write("\n")


def test_planner_reproduces_the_recorded_runner():
    with open(GOLDEN) as f:
        gold = json.load(f)
    cfg, log = gold["config"], []
    p = StagePlanner(cfg["nb"], cfg["rec"], cfg["g"], lambda *a: log.append(list(a)))
    final = _record(p, [tuple(o) for o in gold["ops"]])
    assert len(gold["ops"]) == cfg["nops"] and len(gold["launches"]) > cfg["nops"] // 2
    assert log == gold["launches"]
    assert final == gold["final"]


# ------------------------------------------------------- MLPStepRunner.plan
@pytest.mark.parametrize("prefetch, ipar0", [("serial", 0), ("side", 1)])
def test_step_runner_plan(prefetch, ipar0):
    import torch
    from distributed_tensorflow_example_amd.models.mlp import MLPStepRunner

    tr = SimpleNamespace(ipc_parity=ipar0, device=torch.device("cpu"), B=100)
    run = MLPStepRunner(tr, SimpleNamespace(num_batches=13, rec=78512), steps_per_graph=5, prefetch=prefetch)
    i, j = ipar0, ipar0 ^ 1
    assert run.plan(12) == [(0, 5, 0, (5, 5), i), (5, 5, 1, (10, 2), j), (10, 2, 0, (12, 5), i)]
    run.cursor = 9
    plan = run.plan(12)
    assert plan == [(9, 5, 0, (1, 5), i), (1, 5, 1, (6, 2), j), (6, 2, 0, (8, 5), i)]
    keys = [run._key(b0, g, par, ipar) for b0, g, par, _, ipar in plan]
    assert keys == ([(9, 5, i), (1, 5, j), (6, 2, i)] if prefetch == "serial" else [(5, 0, i), (5, 1, j), (2, 0, i)])
    assert run.cursor == 9 and tr.ipc_parity == ipar0       # planning moves nothing


if __name__ == "__main__":
    _regenerate(os.path.abspath(sys.argv[1]))
