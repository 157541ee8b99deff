"""The closed loops whose results tests/golden/agents_none_loops.npz pins: runs of ClosedLoopRunner WITHOUT agents=, recorded on the
commit before fp_obstacles_from_plans existed.  Only interfaces that commit had are used here, so the same function produced the
recording and reproduces it (tests/test_gpu_agents.py compares the bytes)."""
import numpy as np

KEYS = ("done", "cycles", "ego", "t_now", "cart")


def run_all(engine):
    """-> {"<loop>/<key>": array}"""
    import fallback_cases as FC
    from fiss_plus_planner_amd import synth
    from fiss_plus_planner_amd.device_batch import ClosedLoopRunner, DeviceBatch
    from fiss_plus_planner_amd.fallback import FallbackStop

    out = {}

    def keep(name, res):
        for k in KEYS:
            out[f"{name}/{k}"] = np.ascontiguousarray(getattr(res, k))

    batch, goal = FC.loop_scenario()
    keep("wall fop fallback", ClosedLoopRunner(engine, DeviceBatch(batch), goal, "FOP", fallback=FallbackStop(FC.LOOP_STOP_T)).run(100))
    batch, goal = FC.loop_scenario()
    keep("wall fop unfused", ClosedLoopRunner(engine, DeviceBatch(batch), goal, "FOP", fused=False).run(30))
    for planner, fused in (("FOP", True), ("FISS+", True), ("FISS+", False)):
        b = synth.make_batch(24, 5, 5, 3, 6, 60, True, seed=515, kind=planner)
        keep(f"synth {planner} {'fused' if fused else 'unfused'}", ClosedLoopRunner(engine, DeviceBatch(b), np.full((24, 2), 1e6), planner, fused=fused).run(12))
    b = synth.make_batch(24, 5, 5, 3, 6, 60, True, seed=515, kind="FISS+")
    keep("synth FISS+ fallback", ClosedLoopRunner(engine, DeviceBatch(b), np.full((24, 2), 1e6), "FISS+", fallback=FallbackStop([2.0, 4.0])).run(12))
    return out
