"""Inputs for stage W of the lattice kernel (csrc/frenet_lattice_fused.hip, `// [section WEXIT]`): behind the walk every wavefront reads
the collision masks of the workgroup's slices; when all of them are full the ego's answer is "none" - with no table requested the
assembly and the argmin are skipped, with tables only the argmin.  tests/test_gpu_whole_hit.py runs every case through every kernel
path against the oracle, with tables and without (tests/lattice_quiet.py); tests/test_whole_hit_cpu.py proves with the oracle and the numpy restatement of
stage V's circle (tools/whole_hit_estimate.py, tools/group_hit_estimate.py) what each case is.

The builders are those of tests/sure_hit_cases.py and tests/group_hit_cases.py: the stage stands in the instances that have stage V
(9 x 9 x 7, three and four per CU); 5 x 5 x 5 (two per CU) and a run-time 5 x 4 x 3 are the controls.

CASES: name -> (builder(shape) -> ProblemBatch, kind), kind in
  "V"      stage V ends every end-speed group of every ego: the masks are full before the walk, the verdict is reached
  "walk"   every candidate of every ego collides and every lon profile has two points, but V leaves groups to S, B and N: the walk
           fills the masks, the verdict is reached behind it
  "open"   no ego reaches the verdict: a candidate is free, or a lon profile with M < 2 keeps its mask open
  "mixed"  EGOS names the egos that reach it
"""
import numpy as np

import adversarial as A
import group_hit_cases as H
import prologue_cases as P
import sure_hit_cases as S

SHAPES = S.SHAPES
CONTROLS = ("a box over the first second", "a short horizon among long ones")  # the cases the two control shapes run


def row_zero(batch):
    """A box on the ego at t_now: row 0, where every candidate shares one pose."""
    return S.across(batch, 0)


def late_rows(batch):
    """A box across the line that exists at steps 16, 18 and 20 only (rows 8-10) and covers every lon profile at each of them."""
    pose, dims = batch.obs_pose.copy(), batch.obs_dims.copy()
    for b in range(batch.B):
        s_k = P.lon_positions(batch, b)[:, 16:21]
        lo, hi = np.nanmin(s_k), np.nanmax(s_k)
        c, yaw = S.frame_at(batch, b, 0.5 * (lo + hi))
        S.put(pose, dims, batch, b, 0, 16, c, yaw, (hi - lo + 10.0, 14.0), steps=(16, 18, 20))
    return A._copy(batch, obs_pose=pose, obs_dims=dims)


def line_end(batch, mixed):
    """The egos stand at the end of their line, a box across the end at every step.  mixed = False: the second point of every lon
    profile is off the line (M = 1: no heading, the reference's IndexError -> collision).  mixed = True: the line ends between the
    second points of the slower and the faster end speeds - the faster profiles have M = 1, the slower ones two points and more,
    which stand inside the box.  Every candidate collides in the oracle either way; the profiles with M = 1 are never walked and keep
    their masks open, so the kernel does not reach the verdict: the assembly decides."""
    ego = batch.ego.copy()
    pose, dims = batch.obs_pose.copy(), batch.obs_dims.copy()
    for b in range(batch.B):
        f = int(batch.frame_of[b])
        end = float(batch.knots[f, int(batch.nx[f]) - 1])
        step = np.sort(P.lon_positions(batch, b)[:, 1] - batch.ego[b, 0])  # how far every lon profile moves to its second point
        gap = 0.5 * (step[len(step) // 2 - 1] + step[len(step) // 2]) if mixed else 0.5 * step[0]
        ego[b, 0] = end - gap
        c, yaw = S.frame_at(batch, b, end - 0.5)
        S.put(pose, dims, batch, b, 0, 0, c, yaw, (30.0, 14.0), steps=range(0, batch.T_obs))
    return A._copy(batch, ego=ego, obs_pose=pose, obs_dims=dims)


def nan_pose(batch):
    """The box across the line at an early row has a NaN x in the scenes of the odd egos: a pose that is no number is no state (the
    reference's state_at_time gives None), nothing collides there; the even egos are blocked whole."""
    out = S.across(batch, S.K_EARLY)
    pose = out.obs_pose.copy()
    for b in range(1, out.B, 2):
        pose[int(out.scene_of[b]), :, 0, 0] = np.nan
    return A._copy(out, obs_pose=pose)


def _b(shape, seed):
    return S._base(shape, seed)


CASES = {
    "a box over the first second": (lambda s: H.first_second(_b(s, 9800)), "V"),
    "a box on the ego at t_now": (lambda s: row_zero(_b(s, 9901)), "V"),
    "a box only rows 8-10 reach": (lambda s: late_rows(_b(s, 9902)), "V"),
    "a tight bend": (lambda s: S.tight_bend(_b(s, 9709)), "V"),
    "one candidate of every lon profile passes by 1e-3": (lambda s: S.boundary(_b(s, 9703), 1e-3), "open"),
    "one candidate of every lon profile passes by 1e-5": (lambda s: S.boundary(_b(s, 9703), 1e-5), "open"),
    "along a straight line: the rearmost candidate passes by 1e-5": (lambda s: H.ahead(_b(s, 9811), 1e-5, H.K_AHEAD, False), "open"),
    "along the bend: the rearmost candidate passes by 1e-5": (lambda s: H.ahead(_b(s, 9812), 1e-5, H.K_BEND, True), "open"),
    "the line ends before every second point (M = 1)": (lambda s: line_end(_b(s, 9903), False), "open"),
    "the line ends between the second points (M = 1 and M >= 2)": (lambda s: line_end(_b(s, 9903), True), "open"),
    "a short horizon among long ones": (lambda s: H.short_horizon(_b(s, 9803)), "open"),
    "t_now odd, the table ends inside the horizon": (lambda s: S._variant(s, "t_now odd"), "V"),
    "final_time_step cuts the horizon before the box": (lambda s: H.horizon_cut(_b(s, 9804)), "open"),
    "poses without a state": (lambda s: S._variant(s, "pose without a state"), "mixed"),
    "a NaN pose": (lambda s: nan_pose(_b(s, 9904)), "mixed"),
    "a NaN in v_samples": (lambda s: H.nan_v_sample(_b(s, 9805)), "open"),
    "a NaN in d_samples": (lambda s: S._variant(s, "nan d_sample"), "walk"),
    "a vehicle so small that thr <= 0": (lambda s: H.tiny_vehicle(_b(s, 9806)), "walk"),
    "veh_l < veh_w, a box within the half width ahead": (lambda s: S.wide_vehicle(_b(s, 9704)), "open"),
    "the deciding item in a later chunk of the list": (lambda s: H.later_chunk(_b(s, 9807)), "V"),
}
# the cases built here; the others are cases of tests/sure_hit_cases.py / tests/group_hit_cases.py, seed for seed, whose own CPU files
# prove the separation of every candidate from contact
NEW = ("a box on the ego at t_now", "a box only rows 8-10 reach", "the line ends before every second point (M = 1)",
       "the line ends between the second points (M = 1 and M >= 2)", "a NaN pose")
# "mixed": the egos that reach the verdict (9 x 9 x 7)
EGOS = {"poses without a state": (3, 7), "a NaN pose": (0, 2, 4, 6)}


def build(name, shape):
    fn, kind = CASES[name]
    return fn(shape), kind


def fiss_twin():
    return H.fiss_twin()


def reaches(flags):
    """The kernel's verdict from the oracle's flag words of one ego: every candidate collides and every lon profile has two points (a
    profile with M < 2 is never walked nor marked by V: its mask stays open and the assembly flags it)."""
    return bool(((flags & 4) != 0).all() and ((flags >> 20) >= 2).all())
