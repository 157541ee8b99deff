"""The family of stopping manoeuvres fp_fallback_stop chooses from, described once (the definition: include/frenet_gpu.h).

FallbackStop holds the stop times, the lateral end offsets, the deceleration bound and the road rules the stop obeys (`obey`: then the
call is fp_fallback_stop_rules), validates them without a device and builds the call's ctypes struct for either memory space, like the
rule descriptions in rules.py.
"""
from __future__ import annotations

import math

import numpy as np

from . import _abi
from . import rules as _rules


class FallbackStop:
    """FallbackStop(stop_times, d_targets=None, max_decel=inf, obey=()): candidate f = i_d * n_stop + i_T brakes to v = 0 within
    stop_times[i_T] and ends at lateral offset d_targets[i_d] (NaN = the ego's own d0: stay where you are).  d_targets=None means
    [nan, *batch.d_samples], resolved per batch by targets().  obey: any subset of the names in rules.TABLE - the clear stops are then
    ranked by those rules (fp_fallback_stop_rules: a clean stop before a violating one, the gentlest clean stop, else the fewest rules
    broken and the hardest brake); the batch must carry each rule's data when the call is made (rules_for).  obey=(): fp_fallback_stop."""

    def __init__(self, stop_times, d_targets=None, max_decel: float = math.inf, obey=()):
        asked = () if obey is None else (obey,) if isinstance(obey, str) else tuple(obey)
        for n in asked:
            if n not in _rules.by_name:
                raise ValueError(f"FallbackStop: unknown rule {n!r} in obey (rules are a subset of {tuple(_rules.by_name)})")
        self.obey = tuple(n for n in _rules.by_name if n in asked)  # (the order the rules run in)
        t = np.atleast_1d(np.asarray(stop_times, dtype=np.float64))
        if t.ndim != 1 or t.size < 1:
            raise ValueError("FallbackStop: stop_times must be a non-empty 1-d sequence")
        for i, v in enumerate(t):
            if not (math.isfinite(v) and v > 0.0) or (i > 0 and not v > t[i - 1]):
                raise ValueError(f"FallbackStop: stop_times[{i}]={v} must be finite, > 0 and above stop_times[{i - 1}] (strictly ascending)")
        if d_targets is not None:
            d = np.atleast_1d(np.asarray(d_targets, dtype=np.float64))
            if d.ndim != 1 or d.size < 1:
                raise ValueError("FallbackStop: d_targets must be None or a non-empty 1-d sequence")
            if np.isinf(d).any():
                raise ValueError("FallbackStop: d_targets must be finite (NaN = the ego's own d0)")
            self._check_size(d.size, t.size)
        else:
            d = None
        max_decel = float(max_decel)
        if not max_decel > 0.0:
            raise ValueError(f"FallbackStop: max_decel={max_decel} must be > 0 (inf = no limit)")
        self.stop_times, self.d_targets, self.max_decel = np.ascontiguousarray(t), None if d is None else np.ascontiguousarray(d), max_decel

    @staticmethod
    def _check_size(n_d: int, n_stop: int) -> None:
        if n_d * n_stop > _abi.FP_MAX_FALLBACK:
            raise ValueError(f"FallbackStop: {n_d} lateral targets x {n_stop} stop times = {n_d * n_stop} candidates exceed FP_MAX_FALLBACK ({_abi.FP_MAX_FALLBACK})")

    def targets(self, batch) -> np.ndarray:
        """The lateral end offsets for `batch`: d_targets, or [nan, *batch.d_samples]."""
        d = self.d_targets if self.d_targets is not None else np.concatenate([[np.nan], np.asarray(batch.d_samples, dtype=np.float64)])
        self._check_size(d.size, self.stop_times.size)
        return np.ascontiguousarray(d)

    def n_candidates(self, batch) -> int:
        return int(self.targets(batch).size * self.stop_times.size)

    def rules_for(self, batch, who: str = "FallbackStop") -> tuple:
        """The obeyed rules in the order they run; ValueError (rules.missing) for a rule `batch` carries no data for."""
        return _rules.check_names(self.obey, batch, f"{who}(obey=...)")

    def points_max(self, tick_t: float) -> int:
        """The series points the longest stop time needs (what fp_params.points_max must cover on a device call)."""
        return int(math.ceil(float(self.stop_times[-1]) / float(tick_t)))

    def struct(self, batch, addr) -> _abi.FpFallback:
        """The call's fp_fallback; addr(name, array) = the address of that array in the caller's memory space ("fallback_d" / "fallback_T")."""
        d = self.targets(batch)
        return _abi.FpFallback(int(d.size), int(self.stop_times.size), addr("fallback_d", d), addr("fallback_T", self.stop_times), self.max_decel)
