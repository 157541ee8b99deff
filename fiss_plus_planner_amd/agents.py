"""Egos that see each other's plans, described once (fp_obstacles_from_plans; the definition: include/frenet_gpu.h).

AgentGroups holds the groups - member k of a group owns obstacle column col_base + k of the scene of every member of its group -, the
rows written per member and the tail rule; it validates them against a batch without a device (check), builds the call's ctypes struct
for either memory space (struct, like FallbackStop.struct) and makes a batch in which every member owns a scene to be written into
(attach).
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import _abi

TAILS = {"none": _abi.FP_TAIL_NONE, "hold": _abi.FP_TAIL_HOLD, "coast": _abi.FP_TAIL_COAST}


class AgentGroups:
    """AgentGroups(groups, n_rows, tail="coast", col_base=0): groups = a list of lists of ego indices (an ego in at most one group);
    n_rows = rows written per member from row t_now (at least the longest plan's points + 1 covers the next cycle's whole check
    horizon); tail = what a column holds beyond its plan's last point: "none" no pose, "hold" the last pose, "coast" the last step
    repeated."""

    def __init__(self, groups, n_rows: int, tail: str = "coast", col_base: int = 0):
        if isinstance(tail, str):
            if tail not in TAILS:
                raise ValueError(f"AgentGroups: tail={tail!r} is not one of {tuple(TAILS)}")
            tail = TAILS[tail]
        if int(tail) not in TAILS.values():
            raise ValueError(f"AgentGroups: tail={tail} is not one of FP_TAIL_*")
        if int(n_rows) <= 0:
            raise ValueError(f"AgentGroups: n_rows={n_rows} must be > 0")
        if int(col_base) < 0:
            raise ValueError(f"AgentGroups: col_base={col_base} must be >= 0")
        self.groups = [[int(e) for e in g] for g in groups]
        self.n_rows, self.tail, self.col_base = int(n_rows), int(tail), int(col_base)
        self.group_ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(g) for g in self.groups])]), dtype=np.int32)
        self.members = np.ascontiguousarray([e for g in self.groups for e in g], dtype=np.int32)

    G = property(lambda self: len(self.groups))
    n_members = property(lambda self: int(self.members.size))
    largest = property(lambda self: max((len(g) for g in self.groups), default=0))

    def check(self, batch, best_idx=None, skip=None) -> None:
        """The checks of the host path (FP_MEM_HOST), restated without a device: ValueError naming the group, member or ego."""
        B, S, n_obs = int(batch.B), int(batch.S), int(batch.n_obs)
        group_of, member_of = {}, {}
        for g, members in enumerate(self.groups):
            if self.col_base + len(members) > n_obs:
                raise ValueError(f"AgentGroups: group {g}: col_base + group size = {self.col_base} + {len(members)} exceeds n_obs = {n_obs}")
        for g, members in enumerate(self.groups):
            for k, e in enumerate(members):
                if not 0 <= e < B:
                    raise ValueError(f"AgentGroups: member {k} of group {g} is ego {e}, outside 0 .. B-1 (B={B})")
                if e in group_of:
                    raise ValueError(f"AgentGroups: ego {e} is a member of group {group_of[e]} and of group {g}")
                group_of[e] = g
                sc = int(batch.scene_of[e])
                if sc < 0:
                    raise ValueError(f"AgentGroups: member {k} of group {g} (ego {e}) has no scene (scene_of = {sc})")
                if sc >= S:
                    raise ValueError(f"AgentGroups: scene_of[{e}]={sc} out of range")
                if sc in member_of:
                    raise ValueError(f"AgentGroups: ego {member_of[sc]} and ego {e} share scene {sc} (every member needs a scene of its own)")
                member_of[sc] = e
        if best_idx is not None:
            bi = np.asarray(best_idx)
            for b in range(B):
                if bi[b] >= batch.C and not (skip is not None and skip[b]):
                    raise ValueError(f"AgentGroups: best_idx of ego {b} = {int(bi[b])} is outside the lattice (nd*nv*nt = {batch.C})")

    def struct(self, batch, addr) -> _abi.FpAgents:
        """The call's fp_agents; addr(name, array) = the address of that array in the caller's memory space ("agents_group_ptr" /
        "agents_members")."""
        return _abi.FpAgents(self.G, self.n_members, addr("agents_group_ptr", self.group_ptr), addr("agents_members", self.members) if self.n_members else None,
                             self.col_base, self.n_rows, self.tail, 0)

    def attach(self, batch, T_obs: int, extra_cols: int = 0):
        """A ProblemBatch in which every member owns a fresh scene of T_obs rows: n_obs = max(the batch's, col_base + the largest group +
        extra_cols); the agent columns of a member's scene (col_base + k, k < its group's size) have obs_dims = (veh_l, veh_w); every pose
        of a fresh scene is invalid and its final_time_step = T_obs, except that the columns of the member's old scene (at most col_base
        of them: they sit in front of the agent columns) are copied with their poses and sizes.  Non-members keep their scenes - the
        same indices, rows and columns, the added rows and columns invalid.  Polygon columns and tracks are carried over, the new
        columns being rectangles without a track."""
        T_obs, extra_cols = int(T_obs), int(extra_cols)
        if extra_cols < 0:
            raise ValueError(f"AgentGroups.attach: extra_cols={extra_cols} must be >= 0")
        S0, T0, n0 = int(batch.S), int(batch.T_obs), int(batch.n_obs)
        if T_obs < 1 or (S0 > 0 and n0 > 0 and T_obs < T0):
            raise ValueError(f"AgentGroups.attach: T_obs={T_obs} must be >= 1 and not below the batch's T_obs={T0}")
        seen = {}
        for g, members in enumerate(self.groups):
            for k, e in enumerate(members):
                if not 0 <= e < batch.B:
                    raise ValueError(f"AgentGroups: member {k} of group {g} is ego {e}, outside 0 .. B-1 (B={batch.B})")
                if e in seen:
                    raise ValueError(f"AgentGroups: ego {e} is a member of group {seen[e]} and of group {g}")
                seen[e] = g
        n = max(n0 if S0 > 0 else 0, self.col_base + self.largest + extra_cols)
        S = S0 + self.n_members
        pose = np.zeros((S, T_obs, n, 4))
        dims = np.zeros((S, n, 2))
        fts = np.full(S, T_obs, dtype=np.int32)
        if S0 > 0 and n0 > 0:
            pose[:S0, :T0, :n0] = batch.obs_pose
            dims[:S0, :n0] = batch.obs_dims
        fts[:S0] = batch.final_time_step
        poly = nvert = None
        if batch.obs_nvert is not None:
            poly = np.zeros((S, n) + batch.obs_poly.shape[2:])
            nvert = np.zeros((S, n), dtype=np.int32)
            poly[:S0, :n0], nvert[:S0, :n0] = batch.obs_poly, batch.obs_nvert
        model = state = tframe = None
        if batch.track_model is not None:
            model, state = np.zeros((S, n), dtype=np.int32), np.zeros((S, n, 6))
            model[:S0, :n0], state[:S0, :n0] = batch.track_model, batch.track_state
            tframe = np.zeros(S, dtype=np.int32)
            if batch.track_frame is not None:
                tframe[:S0] = batch.track_frame
        scene_of = np.array(batch.scene_of, dtype=np.int32, copy=True)
        s = S0
        for members in self.groups:
            for e in members:
                old = int(batch.scene_of[e])
                if old >= 0 and n0 > 0:
                    if n0 > self.col_base:
                        raise ValueError(f"AgentGroups.attach: ego {e}'s scene {old} has {n0} columns, more than col_base={self.col_base}: they would be overwritten")
                    pose[s, :T0, :n0], dims[s, :n0] = batch.obs_pose[old], batch.obs_dims[old]
                    if nvert is not None:
                        poly[s, :n0], nvert[s, :n0] = batch.obs_poly[old], batch.obs_nvert[old]
                    if model is not None:
                        model[s, :n0], state[s, :n0] = batch.track_model[old], batch.track_state[old]
                if tframe is not None:
                    tframe[s] = batch.track_frame[old] if old >= 0 and batch.track_frame is not None else batch.frame_of[e]
                dims[s, self.col_base:self.col_base + len(members)] = (batch.veh_l, batch.veh_w)
                scene_of[e] = s
                s += 1
        out = dataclasses.replace(batch, scene_of=scene_of, obs_pose=pose, obs_dims=dims, final_time_step=fts, obs_poly=poly, obs_nvert=nvert,
                                  track_model=model, track_state=state, track_frame=tframe, meta=dict(batch.meta))
        return out
