"""What a granule-gather pass of the persistent fp32 MLP step issues, read from
the code generated for gfx950 (scripts/probes/gather_pass_shape.py; no GPU).

The source said "all in flight" before, while the generated loop waited for
every slot's two loads before it issued the next slot's, so the check is on
the assembly: in bench.py's instantiation the E1 loop issues the loads of all
its NQ - 1 live slots and the E2 loop those of a whole group before the first
wait on a load."""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ = 4       # csrc/kernels/mlp_persist_f32.hip: feature slices (E1 slots)
E2_GRP = 4   # its E2 group size


def _probe():
    spec = importlib.util.spec_from_file_location(
        "gather_pass_shape", os.path.join(REPO, "scripts", "probes", "gather_pass_shape.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_constants_match_the_kernel():
    src = open(os.path.join(REPO, "csrc", "kernels", "mlp_persist_f32.hip")).read()
    assert f"constexpr int NQ = {NQ};" in src
    assert f"constexpr int E2_GRP = {E2_GRP};" in src


def test_flagship_gather_loads_in_flight():
    probe = _probe()
    if probe.hipcc() is None:
        pytest.skip("hipcc not found")
    asm = probe.compile_asm()
    rep = probe.report(asm, probe.FLAGSHIP)
    assert len(rep) == 1, list(rep)
    (name, loops), = rep.items()
    print(name, loops)
    assert len(loops) == 2, loops
    e1, e2 = loops
    # the parent (one divergent region per slot, a vmcnt(0) in each): 2 and 2
    assert e1["loads_before_wait"] >= 2 * (NQ - 1), e1
    assert e2["loads_before_wait"] >= 2 * E2_GRP, e2
    regs = probe.registers(asm)[name]
    assert regs["spill"] == 0 and regs["scratch"] == 0, regs
