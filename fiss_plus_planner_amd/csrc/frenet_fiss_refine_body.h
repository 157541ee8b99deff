// frenet_fiss_refine_body.h - the body of the FISS+ refinement kernels (frenet_fiss.hip), included once per kernel function:
//   FP_REFINE_RULES 0: fiss_refine_kernel<NCH>(FissArgs fa, ...)             - fp_plan_fiss / fp_plan_fiss_step
//   FP_REFINE_RULES 1: fiss_refine_rules_kernel<NCH>(FissRulesArgs fa, ...)  - fp_plan_fiss_rules: a popped candidate whose own word is
//     feasible is also checked against the enforced rules (wave_rule_word) by the wavefront that validated it, and the loop consumes the
//     resulting word - FP_FLAG_BOUNDARY counting as a constraint bit.  The rules' tables are staged beside the spline by the staging
//     wavefronts, behind the refinement's own LDS layout (fa.rules_off).
// Two kernel FUNCTIONS, not two instances of one template: the first one's text - and with it its code, registers and spills - stays what
// it was before the second existed.  No include guard: the text is meant to be included twice.
    constexpr int kPts = NCH * kWave;  // points per trajectory this instance holds
#if defined(FP_PHASE_STAMPS)
    const long long t_begin = wall_clock64();
#else
    const long long t_begin = dur ? wall_clock64() : 0;
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const KernelArgs& ka = fa.ka;
    const fp_params& p = ka.p;
    const fp_batch& bt = ka.b;
    const int b = perm ? perm[blockIdx.x] : (int)blockIdx.x;  // launch order: longest egos first when the host has one
    // Timing diagnostic (tools/refine_stamps.py, -DFP_PHASE_STAMPS): thread 0 leaves 10 ns ticks since the workgroup started in
    // columns 112.. of the last row of the ego's series block (sparse layout, stride 128); column 112 = the absolute start.
#if defined(FP_PHASE_STAMPS)
#define FP_RSTAMP(k) do { if (threadIdx.x == 0 && fa.io.best_traj) fa.io.best_traj[((size_t)b * FP_ARR_COUNT + 15) * fa.io.traj_stride + 112 + (k)] = (k) == 0 ? (double)(t_begin & 0xFFFFFFFFFFll) : (double)(wall_clock64() - t_begin); } while (0)
#else
#define FP_RSTAMP(k) do { } while (0)
#endif
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    constexpr int kThreads = kWave * kRefineWaves;
    const int32_t* ijk = fa.io.best_ijk + (size_t)b * 3;
    const int R = fa.opts.max_refine_iters;
    if (ijk[0] < 0 || R <= 0) {  // nothing found by the coarse search: plan() returns None
        if (tid == 0 && dur) dur[b] = 0;
        if (fa.io.best_traj) {   // NaN series, flag word 0
            KernelArgs kw = ka;
            kw.r.best_traj = fa.io.best_traj;
            kw.r.best_flags = fa.io.best_flags;
            kw.r.traj_stride = fa.io.traj_stride;
            kw.r.traj_sparse = fa.io.traj_sparse;
            const double none = __builtin_nan("");
            if (wave == 0) winner_series_wave(kw, b, b, false, none, none, none, lane, SplineLds{nullptr, nullptr, 0, 0});
        }
        // fp_plan_fiss_step: the hand-over of an ego without a trajectory (R > 0: with R == 0 this kernel is not launched) - "no solution"
        if (ka.has_loop && tid == 0 && R > 0) {
            int off = (int)offsetof(FissArgs, ka);
            asm volatile("" : "+s"(off) : : "memory");
            const KernelArgs& kl = *(const KernelArgs*)((const unsigned char*)__builtin_amdgcn_kernarg_segment_ptr() + off);
            const double none = __builtin_nan("");
            advance_ego_to(kl, b, none, none, none, kl.loop);
        }
        return;
    }
    const int f = bt.frame_of[b];
    const int nx = bt.nx[f];
    const int verdict_off = refine_lds_bytes(bt.NX, pt_rows_max * bt.n_obs, kPts) - 32 - kRefineWaves * 2 * kQueue - 4 * (kHot + 4);
    RefineLds L;
    L.S = (double*)smem;
    L.xy = (double2*)(L.S + kRefineS) + wave * kPts;  // one Cartesian scratch row per wavefront
    L.xyf = (float2*)(L.S + kRefineS + 2 * kPts * kRefineWaves) + wave * kPts;
    L.knots = L.S + refine_spline_off(kPts);
    L.queue = (uint16_t*)(smem + verdict_off + 32) + wave * kQueue;
    L.hot = (int*)(smem + verdict_off + 32 + kRefineWaves * 2 * kQueue);  // [kHot] pairs + [1] count
    if (tid == 0) L.hot[kHot] = 0;  // (the barrier behind the rounds orders it before the first validation)
    L.coef = L.knots + nx;
    // Order of the prologue: wavefront 0 runs the refinement rounds (they only need the ego state: the power sums of a probe's
    // horizon come in closed form) WHILE wavefronts 1..3 stage the spline and the pair table; then the candidate list goes through
    // LDS to every wavefront.  The rounds are ~half of the kernel's instructions: running them once instead of
    // four times is what matters (the kernel is instruction-issue bound), hiding them behind the staging is a bonus.
    const double* gk = bt.knots + (size_t)f * bt.NX;
    const double* gc = bt.coef + (size_t)f * 8 * bt.NX;
    L.pt = nullptr;
    L.ox = gc[0];                       // x, y of the first knot
    L.oy = gc[(size_t)4 * bt.NX];
    const int sc0 = bt.scene_of[b];
    L.scene = sc0;
    L.t_now = bt.t_now[b];
    L.horizon_cap = sc0 >= 0 ? bt.final_time_step[sc0] - L.t_now : 0;
    int pt_rows = 0;
    if (sc0 >= 0 && bt.n_obs > 0 && pt_rows_max > 0) {
        int h = L.horizon_cap;
        if (h > kPts) h = kPts;
        if (h > bt.T_obs - L.t_now) h = bt.T_obs - L.t_now;
        pt_rows = h > 0 ? (h + p.check_stride - 1) / p.check_stride : 0;  // <= pt_rows_max by construction
        L.pt = (float4*)(L.S + refine_pt_off(bt.NX, kPts));
    }
    const double nan = __builtin_nan("");
    double eg[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) eg[m] = bt.ego[(size_t)b * 6 + m];
    const double target_speed = bt.target_speed[b];
    double x[3], res[3], lo[3], hi[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        x[m] = fa.io.end_state[(size_t)b * 3 + m];
        res[m] = fa.io.samp_res[(size_t)b * 3 + m];
        lo[m] = fa.io.samp_min[(size_t)b * 3 + m];
        hi[m] = fa.io.samp_max[(size_t)b * 3 + m];
    }
    const double coarse_x[3] = {x[0], x[1], x[2]};
    double* cand = (double*)(smem + verdict_off + 32);  // [64][4] + {ncand, coarse cost}: the queues' bytes, free until validation
    if (wave > 0) {
        const int stid = tid - kWave;
        constexpr int kStagers = kThreads - kWave;
        for (int i = stid; i < nx; i += kStagers) L.knots[i] = gk[i];
        for (int i = stid; i < 8 * nx; i += kStagers) {
            const int r = i / nx, c = i - r * nx;
            L.coef[r * nx + c] = gc[(size_t)r * bt.NX + c];
        }
        // fp32 broad-phase table of every (checked row, obstacle) pair the collision horizon can touch, once per ego: the
        // validation loop may visit the same pair for up to 21 trajectories
        if (L.pt) {
            const int t0 = L.t_now;
            const double* scene = bt.obs_pose + (size_t)sc0 * bt.T_obs * bt.n_obs * 4;
            const double* gd = bt.obs_dims + (size_t)sc0 * bt.n_obs * 2;
            const double veh_hl = 0.5 * p.veh_l, veh_hw = 0.5 * p.veh_w;
            const double r_ego = sqrt(fma(veh_hl, veh_hl, veh_hw * veh_hw));
            for (int e = stid; e < pt_rows * bt.n_obs; e += kStagers) {
                const int r = e / bt.n_obs, j = e - r * bt.n_obs;
                const double4 ps = *(const double4*)(scene + ((size_t)(r * p.check_stride + t0) * bt.n_obs + j) * 4);
                const double hl = 0.5 * gd[2 * j], hw = 0.5 * gd[2 * j + 1];
                const double rx = ps.x - L.ox, ry = ps.y - L.oy;
                // padding: 1 cm + 2e-6 of the coordinate magnitude dwarfs the fp32 rounding of rx, ry, the pose and the sum
                const double R = r_ego + sqrt(fma(hl, hl, hw * hw)) + 1e-2 + 2e-6 * (fabs(rx) + fabs(ry));
                float R2 = (float)(R * R * (1.0 + 1e-5));
                if (ps.w == 0.0 || !(R2 >= 0.0f)) R2 = -1.0f;  // absent at this step (or NaN size): never passes
                L.pt[e] = make_float4((float)rx, (float)ry, R2, __int_as_float((r * p.check_stride) | (j << 8)));
            }
        }
#if FP_REFINE_RULES
        {  // the rules' own tables, as rules_eval_kernel stages them
            const RulesEvalArgs& a = fa.rules;
            const int NX = bt.NX, cap = points_cap(p);
            const RuleLds T = rule_lds((double*)(smem + fa.rules_off), a.on, NX, cap);
            if (a.on & FP_RULE_LIMIT) {
                const double* gl = a.v_limit + (size_t)f * NX;
                for (int i = stid; i < nx; i += kStagers) T.lim[i] = i + 1 < nx ? gl[i] : __builtin_inf();  // (the last knot starts no segment)
            }
            if (a.on & FP_RULE_BOUNDARY) stage_corridor(gk, a.left + (size_t)f * NX, a.right + (size_t)f * NX, nx, nullptr, T.l0, T.l1, T.r0, T.r1, stid, kStagers);
            if (a.on & FP_RULE_GATE) {
                if (wave == 1) {  // the gate lines with the waiver folded in
                    double g = __builtin_nan("");
                    if (lane < a.gate_stride) {
                        g = a.gate_s[(size_t)f * a.gate_stride + lane];
                        if (gate_waived(a.max_decel, eg[1], eg[0] + a.gate_front, g)) g = __builtin_nan("");
                    }
                    if (lane < FP_MAX_GATES) T.line[lane] = g;
                }
                const uint32_t* closed = a.closed + (size_t)f * a.T_gate;
                for (int i = stid; i < cap; i += kStagers) T.word[i] = gate_word(closed, (long long)L.t_now + 1 + i, a.T_gate - 1);
            }
            if ((a.on & FP_RULE_GAP) && sc0 >= 0 && bt.n_obs > 0) {
                const double* gd = bt.obs_dims + (size_t)sc0 * bt.n_obs * 2;
                for (int j = stid; j < bt.n_obs; j += kStagers) {
                    const double hl = 0.5 * gd[2 * j], hw = 0.5 * gd[2 * j + 1];
                    T.dim[4 * j] = hl;
                    T.dim[4 * j + 1] = hw;
                    T.dim[4 * j + 2] = sqrt(fma(hl, hl, hw * hw));
                    T.dim[4 * j + 3] = 0.0;
                }
            }
        }
#endif
#if defined(FP_RABL) && FP_RABL == 3  // timing ablation: staging only
    } else if (false) {
#else
    } else {
#endif
        // The evaluations form a dependent chain (~2.3 us each on a lone wavefront), so the cost of the CURRENT point x rides along
        // with the six probes around it (lanes >= 6 price x itself): that is the coarse winner's cost in round 0 and the previous
        // round's step afterwards - R + 1 evaluations in the chain instead of 2 R + 1.
        double coarse_cost0 = nan;
        bool have_coarse = false;
        int pending = -1;  // the lane whose trajectory (= x) still waits for its cost
        double my_x[3] = {nan, nan, nan}, my_cost = nan;  // lane c = refinement trajectory c (generation order)
        int ncand = 0;
        for (int r = 0; r < R; ++r) {
            // lanes 0..5: the six probes, lane 6: x itself (role 0: longitudinal half + recombination); lanes 8..14: their lateral halves
            const int pk = lane & 7, dim = pk >> 1;
            double xp[3] = {x[0], x[1], x[2]};
            if (pk < 6) {
                xp[dim] += (pk & 1) ? res[dim] : -res[dim];
#pragma unroll
                for (int m = 0; m < 3; ++m) xp[m] = fmin(fmax(xp[m], lo[m]), hi[m]);  // np.clip
            }
            const bool bad = lane < 6 && (!(xp[0] == xp[0]) || !(xp[1] == xp[1]) || !(xp[2] == xp[2]));
            if (__ballot(bad)) break;
            const double cp = analytic_cost_two_lanes(p, eg, target_speed, xp, (lane >> 3) & 1, kPts);  // valid in lanes 0..6 (6: the cost of x itself)
            {
                const double cx0 = __shfl(cp, 6, kWave);
                if (!have_coarse) { coarse_cost0 = cx0; have_coarse = true; }
                if (lane == pending) my_cost = cx0;
                pending = -1;
            }
            for (int k = 0; k < 6; ++k) {  // hand probe k to lane ncand + k
                const double c = __shfl(cp, k, kWave), a0 = __shfl(xp[0], k, kWave), a1 = __shfl(xp[1], k, kWave), a2 = __shfl(xp[2], k, kWave);
                if (lane == ncand + k) { my_cost = c; my_x[0] = a0; my_x[1] = a1; my_x[2] = a2; }
            }
            ncand += 6;
            double g[3], nrm2 = 0.0;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const double Jl = __shfl(cp, 2 * m, kWave), Jr = __shfl(cp, 2 * m + 1, kWave);
                const double xl = __shfl(xp[m], 2 * m, kWave), xr = __shfl(xp[m], 2 * m + 1, kWave);
                g[m] = (Jr - Jl) / (xr - xl);
                nrm2 += g[m] * g[m];
            }
            const double nrm = sqrt(nrm2);
            double xn[3];
            bool nan_step = false;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                res[m] *= fa.opts.decaying_factor;  // decays in place, like the reference's aliasing of sampling_res (:282)
                xn[m] = x[m] - res[m] * g[m] / nrm;
                xn[m] = fmin(fmax(xn[m], lo[m]), hi[m]);
                nan_step |= !(xn[m] == xn[m]);
            }
            if (nan_step) break;  // zero gradient: the reference raises inside np.arange(nan); refinement stops here
            if (lane == ncand) { my_x[0] = xn[0]; my_x[1] = xn[1]; my_x[2] = xn[2]; }
            pending = ncand;  // priced with the next round's probes, or below
            ncand += 1;
            x[0] = xn[0]; x[1] = xn[1]; x[2] = xn[2];
        }
        if (!have_coarse || pending >= 0) {  // (x is the coarse winner while no round got as far as its evaluation)
            const double cl = analytic_cost(p, eg, target_speed, x, L.S, kPts);
            if (!have_coarse) coarse_cost0 = cl;
            if (lane == pending) my_cost = cl;
        }
        cand[lane * 4] = my_x[0]; cand[lane * 4 + 1] = my_x[1]; cand[lane * 4 + 2] = my_x[2]; cand[lane * 4 + 3] = my_cost;
        if (lane == 0) { cand[4 * kWave] = (double)ncand; cand[4 * kWave + 1] = coarse_cost0; }
    }
    if (wave == 0) FP_RSTAMP(1);
    __syncthreads();
    FP_RSTAMP(2);
    double my_x[3] = {cand[lane * 4], cand[lane * 4 + 1], cand[lane * 4 + 2]};  // lane c = refinement trajectory c (generation order)
    const double my_cost = cand[lane * 4 + 3];
    const int ncand = (int)cand[4 * kWave];
    const double coarse_cost = cand[4 * kWave + 1];
    __syncthreads();  // the queues take their bytes back
#if defined(FP_RABL) && FP_RABL == 1  // timing ablation: rounds + staging only
    return;
#endif
    // refined_trajs.get() in cost order (ties: generation order), :301-323.  Every wavefront holds the same candidate list;
    // the next kRefineWaves trajectories in pop order are checked SPECULATIVELY side
    // by side, one whole wavefront each, and the verdicts are then consumed in pop order exactly like the sequential loop -
    // validated / checks count only what the reference would have popped before its first collision-free trajectory.
    uint32_t* verdict = (uint32_t*)(smem + verdict_off);  // [2][kRefineWaves], double-buffered across groups
    int validated = 0, checks = 0, winner = -1;
#if FP_REFINE_RULES
    // [2][kRefineWaves] beside the verdicts, in the 32 bytes in front of the rules' tables: 1 = the rules rejected a candidate its own word
    // passes; `rejected` counts the consumed ones
    uint32_t* rule_verdict = (uint32_t*)(smem + fa.rules_off) - 2 * kRefineWaves;
    int rejected = 0;
#endif
    bool alive = lane < ncand;
    // Pop order = ascending (cost, generation index): a strict total order unless a cost is NaN, so every lane counts the
    // candidates in front of its own once (register reads, no cross-lane reduction per pop: four 6-step butterflies cost ~1.2 us
    // of every group).  With a NaN cost in the list the butterfly below decides, as it always did.
    int rank = kWave;
    const bool ranked = !__ballot(alive && !(my_cost == my_cost));
    if (ranked) {
        rank = 0;
        for (int j = 0; j < ncand; ++j) {
            const double cj = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_cost), j), __builtin_amdgcn_readlane(__double2loint(my_cost), j));
            rank += (cj < my_cost || (cj == my_cost && j < lane)) ? 1 : 0;
        }
        if (!alive) rank = kWave;
    }
    bool open = true;  // (ranked pops) nothing has ended the loop yet
    for (int grp = 0; winner < 0; ++grp) {
        int pop[kRefineWaves];
        if (ranked) {
#pragma unroll
            for (int u = 0; u < kRefineWaves; ++u) {
                const unsigned long long m = __ballot(rank == grp * kRefineWaves + u);
                int bl = (open && m) ? __ffsll((long long)m) - 1 : -1;
                if (bl >= 0) {
                    const double bc = __shfl(my_cost, bl, kWave);
                    if (bc > coarse_cost) bl = -1;  // `cost > coarse cost` ends the loop (:303-304)
                }
                if (bl < 0) open = false;
                pop[u] = bl;
            }
        } else
#pragma unroll
        for (int u = 0; u < kRefineWaves; ++u) {
            double bc = alive ? my_cost : __builtin_inf();
            int bl = alive ? lane : kWave;
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const double oc = __shfl_xor(bc, off, kWave);
                const int ol = __shfl_xor(bl, off, kWave);
                if (ol < kWave && (bl >= kWave || oc < bc || (oc == bc && ol < bl))) { bc = oc; bl = ol; }
            }
            if (bl >= kWave || bc > coarse_cost) bl = -1;  // queue empty / `cost > coarse cost` ends the loop (:303-304)
            pop[u] = bl;
            if (bl < 0) alive = false;  // nothing further is ever popped
            if (lane == bl) alive = false;
        }
        if (pop[0] < 0) break;
        int mine = pop[0];
#pragma unroll
        for (int u = 1; u < kRefineWaves; ++u) mine = (wave == u) ? pop[u] : mine;
        if (mine >= 0) {
            const double cx[3] = {__shfl(my_x[0], mine, kWave), __shfl(my_x[1], mine, kWave), __shfl(my_x[2], mine, kWave)};
#if defined(FP_PHASE_STAMPS)
            const uint32_t fl = wave_traj_flags<NCH>(ka, b, eg, cx, L, nx, lane, (wave == 0 && grp == 0 && fa.io.best_traj) ? fa.io.best_traj + ((size_t)b * FP_ARR_COUNT + 15) * fa.io.traj_stride + 112 : nullptr, t_begin);
#elif FP_REFINE_RULES
            // (inlined here: as a call the check takes the kernel's argument block through a stack copy - scratch)
            uint32_t fl;
            [[clang::always_inline]] fl = wave_traj_flags<NCH>(ka, b, eg, cx, L, nx, lane);
#else
            const uint32_t fl = wave_traj_flags<NCH>(ka, b, eg, cx, L, nx, lane);
#endif
#if FP_REFINE_RULES && !defined(FP_PHASE_STAMPS)
            {  // a candidate that is feasible by its own word: the enforced rules decide
                uint32_t rule_hit = 0u;
                if (!(fl & FP_FLAG_INFEASIBLE)) {
                    const RuleLds T = rule_lds((double*)(smem + fa.rules_off), fa.rules.on, bt.NX, points_cap(p));
                    fl = wave_rule_word(ka, fa.rules, T, L, b, eg, cx, fl, nx, lane);
                    rule_hit = (fl & FP_FLAG_INFEASIBLE) ? 1u : 0u;
                }
                if (lane == 0) rule_verdict[(grp & 1) * kRefineWaves + wave] = rule_hit;
            }
#endif
            if (lane == 0) verdict[(grp & 1) * kRefineWaves + wave] = fl;
        }
        __syncthreads();
        FP_RSTAMP(3 + (grp < 6 ? grp : 6));
        bool done = false;
#pragma unroll
        for (int u = 0; u < kRefineWaves; ++u) {
            if (done) continue;
            if (pop[u] < 0) { done = true; continue; }
            const uint32_t fl = verdict[(grp & 1) * kRefineWaves + u];
            ++validated;
#if FP_REFINE_RULES
            rejected += (int)rule_verdict[(grp & 1) * kRefineWaves + u];
            if (fl & (FP_FLAG_CONSTRAINTS | FP_FLAG_BOUNDARY)) continue;
#else
            if (fl & FP_FLAG_CONSTRAINTS) continue;
#endif
            ++checks;
            if (!(fl & FP_FLAG_COLLISION)) { winner = pop[u]; done = true; }
        }
        if (done) break;
#if defined(FP_RABL) && FP_RABL >= 4  // timing ablation: at most FP_RABL - 3 validation groups
        if (grp >= FP_RABL - 4) break;
#endif
    }
    if (wave == 0) {
        if (fa.io.trace && lane < R * 7) {
            double* tr = fa.io.trace + ((size_t)b * R * 7 + lane) * 4;
            const bool have = lane < ncand;
            tr[0] = have ? my_x[0] : nan; tr[1] = have ? my_x[1] : nan; tr[2] = have ? my_x[2] : nan; tr[3] = have ? my_cost : nan;
        }
        if (lane == 0) {
            int32_t* s4 = fa.io.stats + (size_t)b * 4;
            s4[1] += ncand;
            s4[2] += validated;
            s4[3] += checks;
#if FP_REFINE_RULES
            if (fa.rejected && rejected != 0) fa.rejected[b] = fa.rejected[b] + rejected;  // (the ego's entry is this workgroup's alone)
#endif
            fa.io.best_cost[b] = coarse_cost;  // same evaluator as the refined costs
        }
        if (winner >= 0 && lane == winner) {
            fa.io.refined[b] = 1;
            fa.io.best_cost[b] = my_cost;
            double* es = fa.io.end_state + (size_t)b * 3;
            es[0] = my_x[0]; es[1] = my_x[1]; es[2] = my_x[2];
        }
    }
    if (tid == 0 && dur) dur[b] = (int)(wall_clock64() - t_begin);  // 10 ns ticks: feeds the next launches' order
    // winner epilogue (what plan() returns) on request: the series of the refined trajectory, or of the coarse winner when no
    // refined one survived.  Every wavefront holds the same candidate list; wavefront 0 writes the series (two time points per
    // lane, no barrier), the others are done.
#if defined(FP_RABL) && FP_RABL == 2  // timing ablation: no series
    return;
#endif
    if ((fa.io.best_traj || ka.has_loop) && wave == 0) {
        double fx[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) fx[m] = winner >= 0 ? __shfl(my_x[m], winner, kWave) : coarse_x[m];
        if (fa.io.best_traj) {
            KernelArgs kw = ka;
            kw.r.best_traj = fa.io.best_traj;
            kw.r.best_flags = fa.io.best_flags;
            kw.r.traj_stride = fa.io.traj_stride;
            kw.r.traj_sparse = fa.io.traj_sparse;
            FP_RSTAMP(10);
            bool long_series = false;
            if constexpr (NCH > 2) {  // more points than the one-chunk writer holds: the chunked writer (frenet_winner.h), same arithmetic per element
                const int n_pts = (fx[2] == fx[2]) ? arange_len(fx[2], p.tick_t) : 0;
                long_series = n_pts > kSeriesChunk && n_pts <= points_cap(p) && (fx[0] == fx[0]) && (fx[1] == fx[1]);
                if (long_series) winner_series_wave_long(kw, b, b, fx[0], fx[1], fx[2], lane, SplineLds{L.knots, L.coef, nx, nx});
            }
            if (!long_series) winner_series_wave(kw, b, b, true, fx[0], fx[1], fx[2], lane, SplineLds{L.knots, L.coef, nx, nx});
            FP_RSTAMP(11);
            FP_RSTAMP(0);
        }
        // fp_plan_fiss_step: the workgroup that settled the ego's trajectory hands the ego over to its next state itself (after the
        // series, which describe the trajectory from the OLD state; every other wavefront of the workgroup is done with the state,
        // and no other workgroup reads it) - no advance_kernel launch behind the pipeline
        // (the hand-over's arguments are re-read from the kernel's argument segment HERE, through a laundered pointer: as ordinary kernel
        // arguments the compiler loads the loop structure's eleven fields at the kernel's start and holds them - 47 more spilled SGPRs
        // and, through their lanes, two spilled VGPRs in a kernel that is at its register budget)
        if (ka.has_loop && lane == 0) {
            int off = (int)offsetof(FissArgs, ka);
            asm volatile("" : "+s"(off) : : "memory");  // (an offset the compiler cannot see through: the loads below depend on it and stay here)
            const KernelArgs& kl = *(const KernelArgs*)((const unsigned char*)__builtin_amdgcn_kernarg_segment_ptr() + off);
            advance_ego_to(kl, b, fx[0], fx[1], fx[2], kl.loop);
        }
    }
