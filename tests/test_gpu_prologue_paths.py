"""GPU: the fused lattice kernel's prologue and group test (csrc/frenet_lattice_fused.hip, sections STAGE .. G) on the inputs at which the
code that deals their work to lanes and wavefronts can go wrong (tests/prologue_cases.py).

* G's indexing   the shaped instances give a lane one obstacle column and step it through the rows, the others take item = pass x threads
                 + thread apart by division: the compiled-in 25 x 50 table; run-time tables that are no multiple of a pass (13 rows x 7
                 obstacles, one obstacle); t_now odd at check stride 2; tables that end inside the horizon; pose rows with valid == 0 and
                 with x = NaN; an ego without a scene in the same launch.
* item order     every other ego stands inside an obstacle: all of its profiles are blocked by the list's first items.
* chunked redo   every (row, obstacle) item survives the group test: more than any instance's list holds.
* cost sums      lon and lat lanes dealt to a wavefront each (shaped) or nv + nd lanes per slice (run-time shape): nd != nv, nt (nv + nd)
                 below 64, between 64 and 128 and above; d_samples descending and with a NaN sample (the ends of d_samples are found by
                 one wavefront in the shaped instances).
* uniforms       values only some wavefronts compute: a line with all knots in one place (bucket width 0), a windowed launch on a
                 220-knot line, veh_l == veh_w.

Every case runs through the two-, three- and four-per-CU instances (tests/lattice_paths.py's MODES, launch counters asserted)
and is compared with the oracle: flag words, Stats and the selected index exact, cost within 1e-9 (lattice_paths.shaped_case)."""
import pytest

import lattice_paths as L
import prologue_cases as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(P.CASES))
def test_prologue_case_through_every_instance(oracle, engine, name):
    batch = P.CASES[name]()
    assert 8 <= batch.B <= 16
    L.shaped_case(oracle, engine, batch, name, L.SHAPE_997 if name in P.SHAPED else None, L.MODES)
