// lbm_launch.hip -- kernel launches (row kernels, frame passes, tile kernel, streaming kernels) and the step loop: the launch unit
// (run_unit: which work goes on which stream; their ordering is lbm_order.hpp's), the lagged lattice.
#include "lbm_host.hpp"

namespace lbmhost {

// Scratch lattices lat[2 .. 2 + n) of the frame passes, allocated on first use: the fused frame passes keep their
// intermediate results in LDS windows whenever those fit, so the default fp32 / fp64 paths never touch a scratch lattice and a
// streaming context holds 2 lattices (3 once the lagged fields have been asked for) instead of 2 + 7 -- 8192^2 fp64: 9.7 GB instead
// of 48.  Only frame_beside, LBM_FLAG_FRAME_UNFUSED / NO_FRAME_LDS, windows that do not fit, and the replay of the lagged lattice
// by single steps go through them.  Zeroed like the lattices themselves (dead reads of ghost positions see numbers); the wait makes
// the memory safe for either stream, once per lattice and context.
int ensure_scratch(lbm_ctx* c, int n) {
    bool fresh = false;
    for (int i = 2; i < 2 + n && i < LAT_LAG; ++i) {
        if (c->lat[i]) continue;
        int rc = alloc_ok(c, c->lat[i].alloc(c->plan.lat_bytes, "scratch lattice of the frame passes"));
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(c->lat[i].get(), 0, c->plan.lat_bytes, c->s_compute));
        rc = solid_copy_links(c, i);   // (solid obstacles: every lattice a step or an export reads carries the link plane)
        if (rc) return rc;
        fresh = true;
    }
    if (fresh) HIP_TRY(c, hipStreamSynchronize(c->s_compute));
    return LBM_OK;
}

// One single step, lat[from] -> lat[to], on local rows row0 + i*stride, i in [0, nrows).
int launch_rows(lbm_ctx* c, int from, int to, int row0, int stride, int nrows, hipStream_t s) {
    if (nrows <= 0) return LBM_OK;
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        const R* src = c->lat[from].as<const R>();
        R* dst = c->lat[to].as<R>();
        const int raw = c->raw[from];
        // the vector kernels: a block per BLK vectors of a row; NT: non-temporal loads and stores
        constexpr int V = 16 / (int)sizeof(R);
        const int nxb = (c->plan.geo.nx / V + BLK - 1) / BLK, nblocks = nxb * nrows;
        const dim3 gvec(nblocks, c->plan.batch);
        auto by_nt = [&](auto&& launch) {
            if (c->plan.use_nt) launch(std::true_type{});
            else launch(std::false_type{});
        };
        if constexpr (VT::SEM == SEM_SOLID) {
            // the wall mode's kernel on either route (with_wall); at rest the one-cell route is k_step_generic below, as without a mask
            bool launched = true;
            with_wall_step<VT>(c, [&](auto wa, const double*) {   // (the mode with the bits of the context's run state)
                constexpr int WALL = decltype(wa)::MODE;
                if (c->plan.use_vec)   // (nx a multiple of the vector width, kernel = AUTO: plan_kernel)
                    by_nt([&](auto nt) {
                        hipLaunchKernelGGL((k_step_solid<R, VT::COLL, decltype(nt)::value, WALL>), gvec, dim3(BLK), 0, s, src, dst, c->plan.geo,
                                           relax_of<R>(c->p), batch_of<R>(c), raw | (c->driven() ? SOLID_DRIVE : 0), row0, stride, nxb, nblocks, wa, drive_of<R>(c));
                    });
                else if (WALL != WALL_REST || c->driven())   // (at rest the kernel with a mode launches for the driving force alone; the closure is a mode)
                    hipLaunchKernelGGL((k_step_generic_wall<R, VT::COLL, WALL>), grid_rows(c, nrows), dim3(BLK), 0, s, src, dst, c->plan.geo,
                                       relax_of<R>(c->p), batch_of<R>(c), raw, row0, stride, wa, drive_of<R>(c));
                else launched = false;
            });
            if (launched) return;
        }
        if (VT::SEM == SEM_GPU && c->plan.use_vec)
            by_nt([&](auto nt) {
                hipLaunchKernelGGL((k_step_vec<R, VT::COLL, V, decltype(nt)::value, VT::TURB>), gvec, dim3(BLK), 0, s, src, dst, c->plan.geo,
                                   relax_of<R>(c->p), batch_of<R>(c), raw, row0, stride, nxb, nblocks);
            });
        else
            hipLaunchKernelGGL((k_step_generic<R, VT::COLL, VT::SEM, VT::TURB>), grid_rows(c, nrows), dim3(BLK), 0, s, src, dst, c->plan.geo,
                               relax_of<R>(c->p), batch_of<R>(c), raw, row0, stride);
    });
}

// One single step on the frame of width W, lat[from] -> lat[to] (one pass of a multi-step; never a raw lattice).
int launch_frame(lbm_ctx* c, int from, int to, int W, hipStream_t s, int elo, int ehi) {
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        constexpr int V = 16 / (int)sizeof(R);
        const int vec_rows = VT::SEM == SEM_GPU && c->plan.use_vec && c->plan.geo.nx % V == 0 ? 1 : 0;   // row strips by vector cells
        const long long cells = (2LL * W + elo + ehi) * (vec_rows ? c->plan.geo.nx / V : c->plan.geo.nx) + 2LL * W * (c->plan.geo.ny - 2 * W);
        if constexpr (sem_multi_step(VT::SEM))
            hipLaunchKernelGGL((k_step_frame<R, VT::COLL, VT::SEM, VT::TURB>), dim3((unsigned)((cells + BLK - 1) / BLK), c->plan.batch), dim3(BLK), 0, s,
                               c->lat[from].as<const R>(), c->lat[to].as<R>(), c->plan.geo, relax_of<R>(c->p), batch_of<R>(c), W, elo, ehi, vec_rows);
    });
}

// The wall frame of a unit of S steps as the fused frame passes cut it (frame_passes): the two row strips in nsegx segments of L
// columns each, the two column strips over the rows [ybeg, yend) in nsegy segments of L rows each, one workgroup per segment (nframe
// of them; 0 when the launch has no frame).  in_lds: the passes keep their intermediate results in LDS windows (frame_lds_fits with
// `budget` bytes, deep_rows and extra); where they do not, the scratch lattices are allocated here.
struct FrameLayout {
    int F, L, nsegx, nsegy, nframe;
    bool in_lds;
};
static int frame_layout(lbm_ctx* c, FrameLayout& fl, int S, int ybeg, int yend, long long budget, bool deep_rows, int extra, bool with_frame = true) {
    fl.F = c->plan.tb_f;
    fl.L = c->plan.frame_seg;
    fl.nsegx = frame_segs(c->plan.geo.nx, fl.L);
    fl.nsegy = frame_segs(yend - ybeg, fl.L);
    fl.nframe = with_frame ? 2 * fl.nsegx + 2 * fl.nsegy : 0;
    fl.in_lds = frame_lds_fits(c->plan, S, deep_rows, extra, budget);
    return with_frame && !fl.in_lds ? ensure_scratch(c, S - 1) : LBM_OK;
}

// extra: rows of the neighbours' side that the row strips own on top of the slab's (see frame_passes)
int launch_frame_multi(lbm_ctx* c, int from, int to, int S, hipStream_t s, bool lo, bool hi, int extra) {
    // (beside the streaming kernel: k_frame_beside has no LDS, its passes go through the scratch lattices)
    const bool beside = c->plan.frame_beside && !lo && !hi && c->plan.batch == 1;
    FrameLayout fl;
    const int rc = frame_layout(c, fl, S, c->plan.tb_f, c->plan.geo.ny - c->plan.tb_f, beside ? 0 : FRAME_LDS_BYTES, lo || hi, extra);
    if (rc) return rc;
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        const FramePtrs<R> fp = frame_ptrs<R>(c, from, to, S);
        if (beside) {   // (Kern::stream only: never with solid obstacles)
            if constexpr (sem_multi_step(VT::SEM, true))
                hipLaunchKernelGGL((k_frame_beside<R, VT::COLL, VT::SEM, VT::TURB>), dim3(fl.nframe), dim3(BLK), 0, s, fp, c->plan.geo, relax_of<R>(c->p), fl.F, S,
                                   fl.nsegx, fl.nsegy, fl.L);
        } else if (!fl.in_lds && c->plan.frame_wide)
            hipLaunchKernelGGL((k_frame_multi<R, VT::COLL, VT::SEM, VT::TURB, 1024>), dim3(fl.nframe, c->plan.batch), dim3(1024), 0, s, fp, c->plan.geo,
                               relax_of<R>(c->p), batch_of<R>(c), fl.F, S, fl.nsegx, fl.nsegy, lo ? 1 + extra : 0, hi ? 1 + extra : 0, fl.L, 0);
        else
            hipLaunchKernelGGL((k_frame_multi<R, VT::COLL, VT::SEM, VT::TURB, BLK>), dim3(fl.nframe, c->plan.batch), dim3(BLK), 0, s, fp, c->plan.geo,
                               relax_of<R>(c->p), batch_of<R>(c), fl.F, S, fl.nsegx, fl.nsegy, lo ? 1 + extra : 0, hi ? 1 + extra : 0, fl.L,
                               fl.in_lds ? 1 : 0);
    });
}

// The one launcher of k_stream: the frame workgroups of fl, then nstrips x nseg streaming segments of the strip plan pl below row ye.
// lo / hi / bands: the interface bands of an edge launch (launch_stream_edges; 0: the segments start at row F).
static int launch_k_stream(lbm_ctx* c, int from, int to, hipStream_t s, int S, const FrameLayout& fl, const StreamPlan& pl, int nseg, int ye,
                           int lo, int hi, int bands, bool xcd_bands) {
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        if constexpr (sem_multi_step(VT::SEM, true))
        hipLaunchKernelGGL((k_stream<R, VT::COLL, VT::SEM, VT::TURB>), dim3(fl.nframe + pl.nstrips * nseg), dim3(ST_NT), 0, s, c->lat[from].as<const R>(),
                           c->lat[to].as<R>(), c->plan.geo, relax_of<R>(c->p), S, fl.F, c->plan.geo.nx - fl.F, ye, pl.nstrips, pl.H, frame_ptrs<R>(c, from, to, S),
                           fl.nframe, fl.nsegx, fl.nsegy, fl.L, fl.in_lds ? 1 : 0, lo, hi, bands, xcd_bands ? 1 : 0);
    });
}

// The kernels with the walls inside: a lone lattice whole (k_stream_walls, or k_stream_pairs) or a slab by k_stream_walls_slab over the
// rows [ybeg, yend) between its edge bands (bands = 0: the bulk launch), or over the interface bands `bands` (bit 0: low, bit 1: high)
// alone, each of which starts elo / ehi rows inside the neighbour's rows (the edge launch).
static int launch_walls(lbm_ctx* c, int from, int to, hipStream_t s, int S, int ybeg, int yend, int bands, int elo, int ehi) {
    const StreamPlan pl = plan_stream(c->plan, S);
    const int xcd = c->plan.xcd_bands ? 1 : 0;
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        if constexpr (VT::SEM == SEM_GPU) {
            const R* src = c->lat[from].as<const R>();
            R* dst = c->lat[to].as<R>();
            if (is_slab(c->plan))
                hipLaunchKernelGGL((k_stream_walls_slab<R, VT::COLL, VT::TURB>), dim3(pl.nstrips * (bands ? (bands & 1) + (bands >> 1) : pl.nsegy)),
                                   dim3(ST_NT), 0, s, src, dst, c->plan.geo, relax_of<R>(c->p), S, pl.nstrips, pl.H, bands ? 0 : xcd, ybeg, yend, bands,
                                   elo, ehi, bands ? c->plan.tb_f : 0);
            else if constexpr (coll_is_prom(VT::COLL)) {   // (not compiled for the promoted operators: plan_kernel refuses stream_pairs with them)
                hipLaunchKernelGGL((k_stream_walls<R, VT::COLL, VT::TURB>), dim3(pl.nstrips * pl.nsegy), dim3(ST_NT), 0, s, src, dst, c->plan.geo,
                                   relax_of<R>(c->p), S, pl.nstrips, pl.H, xcd);
            } else if (c->plan.kern == Kern::stream_pairs)
                hipLaunchKernelGGL((k_stream_pairs<R, VT::COLL, VT::TURB>), dim3(pl.nstrips * pl.nsegy), dim3(64 * pairs_waves(S)), 0, s, src, dst,
                                   c->plan.geo, relax_of<R>(c->p), S, pl.nstrips, pl.H, xcd);
            else
                hipLaunchKernelGGL((k_stream_walls<R, VT::COLL, VT::TURB>), dim3(pl.nstrips * pl.nsegy), dim3(ST_NT), 0, s, src, dst, c->plan.geo,
                                   relax_of<R>(c->p), S, pl.nstrips, pl.H, xcd);
        }
    });
}

int launch_stream(lbm_ctx* c, int from, int to, hipStream_t s, int S, bool with_frame) {
    const int F = c->plan.tb_f, ny = c->plan.geo.ny;
    if (walls_inside(c->plan)) {
        // walls included, no frame at all: the whole lattice in one launch (with_frame), or a slab's rows between its edge bands
        const bool slab = is_slab(c->plan);
        if (slab == with_frame) return fail(c, LBM_ERR_STATE, "internal: the streaming kernel with the walls inside takes a whole lone lattice or a slab's bulk rows");
        return launch_walls(c, from, to, s, S, has_neighbour(c->plan, LBM_SIDE_LOW) ? F : 0, ny - (has_neighbour(c->plan, LBM_SIDE_HIGH) ? F : 0), 0, 0, 0);
    }
    FrameLayout fl;
    const int rc = frame_layout(c, fl, S, F, ny - F, ST_LDS_BYTES, false, 0, with_frame);
    if (rc) return rc;
    const StreamPlan pl = plan_stream(c->plan, S);
    return launch_k_stream(c, from, to, s, S, fl, pl, pl.nsegy, ny - F, 0, 0, 0, c->plan.xcd_bands);
}

// The edge launch of a slab's unit under the streaming kernel: everything but the bulk rows [F, ny - F) x [F, nx - F) -- the wall
// frame (the column strips over the slab's whole height, the row strip of a lid / bottom wall this slab holds) by the frame
// workgroups and, on each side with a neighbour, the F rows next to the interface between the column strips as a short
// streaming segment that starts in the neighbour's rows of the deep halo.  It writes every row the next exchange sends.
// extra: rows of the neighbours' side owned on top (1 for the lagged lattice, see frame_passes).
int launch_stream_edges(lbm_ctx* c, int from, int to, hipStream_t s, int S, bool lo, bool hi, int extra) {
    const int elo = lo ? 1 + extra : 0, ehi = hi ? 1 + extra : 0, bands = (lo ? 1 : 0) | (hi ? 2 : 0);
    // the walls inside: the edge launch is the interface bands alone, over the whole width (side-wall cells in line)
    if (walls_inside(c->plan)) return launch_walls(c, from, to, s, S, 0, 0, bands, elo, ehi);
    const int F = c->plan.tb_f, ny = c->plan.geo.ny;
    FrameLayout fl;
    const int rc = frame_layout(c, fl, S, lo ? -extra : F, hi ? ny + extra : ny - F, ST_LDS_BYTES, false, extra);
    if (rc) return rc;
    return launch_k_stream(c, from, to, s, S, fl, plan_stream(c->plan, S), (lo ? 1 : 0) + (hi ? 1 : 0), ny - F, elo, ehi, bands, false);
}

// The first launch of the streaming kernel in a process costs ~1.4 ms (code upload, 144 KiB of LDS, scratch set-up).  Where the first
// units of a run may go to the tile kernel (tail_tiles: Kern::stream on a lone fp32 lattice) that cost would land in the middle of a
// run -- in the driver's 20 timed steps after a 5-step warm-up, for one -- so lbm_create pays it: one workgroup that returns at once
// (its segment, rows [F, ye = F), is empty).
int warm_stream(lbm_ctx* c) {
    const FrameLayout none{c->plan.tb_f, c->plan.frame_seg, 1, 1, 0, false};
    return launch_k_stream(c, 0, 1, c->s_compute, c->plan.tb_steps, none, StreamPlan{1, 1, 1}, 1, c->plan.tb_f, 0, 0, 0, false);
}

// The bulk launch of a unit (with_frame: and the frame, the unit's only launch) by the context's kernel.
int launch_deep(lbm_ctx* c, int from, int to, hipStream_t s, int steps, bool with_frame) {
    // A short unit of a lone fp32 lattice (the tail of a call: 3 .. 5 steps) goes to the tile kernel: a launch of the streaming
    // kernel costs nearly the same whatever its length (4096^2 fast: 311 us for four steps, 374 for eight), the tile kernel's four
    // steps take ~290 (strict ~300 against ~350): the driver's 20 timed steps, fast 1088 -> 1066 us, strict 1466 -> 1412
    // (profiles/r02_logs/tail_tiles.log)
    switch (c->plan.kern) {
        case Kern::stream:
            if (c->plan.tail_tiles && c->plan.frame_fused && with_frame && steps >= 3 && steps <= 5) break;
            [[fallthrough]];
        case Kern::stream_walls:
        case Kern::stream_pairs: return launch_stream(c, from, to, s, steps, with_frame);
        default: break;
    }
    const int F = c->plan.tb_f, xe = c->plan.geo.nx - F, ye = c->plan.geo.ny - F;
    if (steps < 3 && c->plan.solid_tiles) return fail(c, LBM_ERR_STATE, "internal: solid obstacles have no two-step tile kernel");
    if (steps < 3)
        return launch_variant(c, [&](auto v) {
            using VT = decltype(v);
            using R = typename VT::R;
            constexpr int V = 16 / (int)sizeof(R), TX = tb_txv<VT::TURB>() * V, TY = tb_ty<VT::TURB>();
            const int ntx = (xe - TB_F + TX - 1) / TX, nty = (ye - TB_F + TY - 1) / TY;   // two steps: F = TB_F
            hipLaunchKernelGGL((k_step2_deep<R, VT::COLL, VT::TURB>), dim3(ntx * nty, c->plan.batch), dim3(TB_NT), 0, s, c->lat[from].as<const R>(),
                               c->lat[to].as<R>(), c->plan.geo, relax_of<R>(c->p), batch_of<R>(c), xe, ye, ntx, ntx * nty);
        });
    const int S_tile = steps == 4 || steps == 5 ? steps : 3;
    FrameLayout fl;
    const int rc = frame_layout(c, fl, S_tile, F, c->plan.geo.ny - F, TILE_FRAME_LDS_BYTES, false, 0, with_frame);
    if (rc) return rc;
    return launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        constexpr int V = 16 / (int)sizeof(R);
        auto go = [&](auto steps) {   // (fp64: the x rim of S >= 4 is two vectors wide)
            constexpr int S = decltype(steps)::value, PVC = 16, RV = (S - 1 + V - 1) / V, TX = (PVC - 2 * RV) * V, TY = 512 / PVC - 2 * (S - 1);
            const int ntx = (xe - F + TX - 1) / TX, nty = (ye - F + TY - 1) / TY;
            if constexpr (sem_multi_step(VT::SEM))
            hipLaunchKernelGGL((k_stepS_deep<R, VT::COLL, VT::SEM, S, false, VT::TURB>), dim3(fl.nframe + ntx * nty, c->plan.batch), dim3(512), 0, s,
                               c->lat[from].as<const R>(), c->lat[to].as<R>(), c->plan.geo, relax_of<R>(c->p), batch_of<R>(c), F, xe, ye, ntx, ntx * nty,
                               frame_ptrs<R>(c, from, to, S), fl.nframe, fl.nsegx, fl.nsegy, fl.L, fl.in_lds ? 1 : 0);
        };
        if (S_tile == 4) go(std::integral_constant<int, 4>{});
        else if (S_tile == 5) go(std::integral_constant<int, 5>{});
        else go(std::integral_constant<int, 3>{});
    });
}

// bookkeeping after a launch unit of S steps lat[cur] -> lat[cur ^ 1]
void finish_unit(lbm_ctx* c, int S) {
    c->cur ^= 1;
    c->raw[c->cur] = c->plan.push ? 1 : 0;   // (push scheme: the lattices hold plain populations, nothing to stream at read time)
    c->nsteps += S;
    c->lag = S - 1;
    c->lag_valid = false;
    c->order.set_thin_valid(false);
}

// The frame work of a unit of S steps on route `route` (edges_bulk, fused_frame or frame_passes: unit_route), lat[from] -> lat[to] on
// stream s.  extra: rows of the neighbours' side owned on top (see launch_frame_multi).  The per-pass frame goes through the scratch
// lattices; a slab without the deep halo exchanges one row after every pass but the last.
static int launch_frame_work(lbm_ctx* c, Route route, int from, int to, hipStream_t s, int S, int extra) {
    const bool lo = has_neighbour(c->plan, LBM_SIDE_LOW), hi = has_neighbour(c->plan, LBM_SIDE_HIGH), deep = is_slab(c->plan) && c->plan.deep_halo;
    if (route == Route::edges_bulk) return launch_stream_edges(c, from, to, s, S, lo, hi, extra);
    if (route == Route::fused_frame) return launch_frame_multi(c, from, to, S, s, deep && lo, deep && hi, extra);
    int rc = ensure_scratch(c, 2);
    for (int i = 1; i <= S && rc == LBM_OK; ++i) {
        const int next = i == S ? to : 2 + ((i - 1) & 1), ext = deep ? S - i + extra : 0;
        rc = launch_frame(c, from, next, c->plan.tb_f + S - i, s, lo ? ext : 0, hi ? ext : 0);
        if (rc == LBM_OK && is_slab(c->plan) && !deep && i < S) rc = enqueue_exchange(c, next);
        from = next;
    }
    return rc;
}

// One launch unit of S >= 1 steps, lat[a] (state n) -> lat[b] (state n + S).  It picks the unit's work and hands it to the skeleton
// that orders the two streams (lbm_order.hpp, with the argument why that order is enough):
//   a lone lattice in one launch   all rows (S = 1), or frame and bulk / the walls inside (launch_deep, with_frame) on s_compute;
//   S = 1 on a slab                the edge rows 0 and ny - 1, which read the ghost rows, on s_comm | the interior rows on s_compute;
//   S >= 2 on two streams          the frame work (launch_frame_work) on s_comm | the bulk kernel (launch_deep) on s_compute.
// Bulk: the deep-interior kernel on cells >= tb_f away from walls and slab edges.  Frame: S ordinary single steps on strips of
// decreasing width (tb_f + S - i for pass i; pass i+1 pulls from one cell further out than it writes), through the scratch lattices,
// the last one into lat[b]; under the streaming kernel the frame work of a slab is its edge launch (launch_stream_edges: column
// strips + the interface rows as short streaming segments).  (Running row and column strips as separate launches on separate
// streams was measured and lost 8 %: profiles/r01_logs/perf31.log, perf35.log.)
// rccl_x: the library moves the halos (lbm_step); otherwise the caller has (lbm_step_unit).  The unit's exchange: a raw lattice is
// not streamed and needs none; with the deep halo (MRT_GPU semantics, S >= 2) the S rows next to each interface, of which the row
// strips of pass i use S - i, the unit's only exchange; otherwise one row, unless the last call left it in place, and
// one more after every frame pass but the last (launch_frame_work).
int run_unit(lbm_ctx* c, bool* comm_used, int S, bool rccl_x) {
    const int ny = c->plan.geo.ny, a = c->cur, b = c->cur ^ 1;
    const bool slab = is_slab(c->plan), deep = slab && S > 1 && c->plan.deep_halo;
    const Route route = S > 1 ? unit_route(c->plan, S, false) : Route::one_launch;
    HipDev dev{c};
    int rc;
    if (S > 1 ? route == Route::one_launch : !slab) {
        rc = one_stream_unit(c->order, dev, [&] {
            if (S > 1) return launch_deep(c, a, b, c->s_compute, S, true);
            const int rc1 = launch_rows(c, a, b, 0, 1, ny, c->s_compute);
            return rc1 ? rc1 : periodic_wrap(c, b, c->s_compute);   // (periodic sides: the image cells of the lattice just written)
        });
    } else {
        if (S > 1 && slab && !deep && !rccl_x) return fail(c, LBM_ERR_STATE, "a multi-step unit of a slab needs the deep halo (MRT_GPU semantics) or the in-library exchange");
        const bool exchange = slab && rccl_x && !c->raw[a] && (deep || !c->order.thin_valid());
        // The streaming kernel between slabs: edge launch and bulk launch both become ready when the previous bulk launch ends, and the
        // bulk launch -- one workgroup per CU for its whole run -- must not take the CUs first: the edge workgroups would run last, and
        // the next exchange after them, in the open.  So the bulk launch is held one cross-stream hop behind the edge launch -- when it
        // runs more than one round of workgroups (16384 x 2048 fp32 slab in loopback 319 -> 359 GLUPS, 8192 x 1024 fp64 133 -> 142); a
        // one-round launch does not gain and a short one loses (4096 x 4096 355 -> 351, 4096 x 1024 249 -> 205:
        // profiles/r02_logs/slab_loopback7.log).
        bool hold = false;
        if (route == Route::edges_bulk && c->plan.edge_first) {
            const StreamPlan pl = plan_stream(c->plan, S);
            hold = (long long)pl.nstrips * pl.nsegy > c->plan.ncu;
        }
        rc = two_stream_unit(
            c->order, dev, exchange ? (deep ? S : 1) : 0, hold, S > 1 ? c->plan.tb_f : 1,
            [&] { return deep ? enqueue_deep_exchange(c, a, S) : enqueue_exchange(c, a); },
            [&] { return S > 1 ? launch_frame_work(c, route, a, b, c->s_comm, S, 0) : launch_rows(c, a, b, 0, ny - 1, 2, c->s_comm); },
            [&] { return S > 1 ? launch_deep(c, a, b, c->s_compute, S) : launch_rows(c, a, b, 1, 1, ny - 2, c->s_compute); });
        *comm_used = true;
    }
    if (rc) return rc;
    finish_unit(c, S);
    // a passive scalar (lbm_scalar_begin: a lone lattice, one step per launch) follows the flow step and its wrap, on s_compute
    return c->scalar.active ? scalar_step(c) : LBM_OK;
}

// Recompute the lattice of the step before the last into lat[LAT_LAG] (see lbm_ctx::lag); returns the index of the lattice
// whose gathered populations are the state the LAST iteration started from.
int prev_lattice(lbm_ctx* c, int* which) {
    if (c->nsteps == 0) { *which = c->cur; return LBM_OK; }
    if (c->lag == 0) { *which = c->cur ^ 1; return LBM_OK; }
    *which = LAT_LAG;
    if (c->lag_valid) return LBM_OK;
    if (!c->lat[LAT_LAG]) {
        int rc = alloc_ok(c, c->lat[LAT_LAG].alloc(c->plan.lat_bytes, "lag lattice"));
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(c->lat[LAT_LAG].get(), 0, c->plan.lat_bytes, c->s_compute));
        rc = solid_copy_links(c, LAT_LAG);
        if (rc) return rc;
    }
    const int k = c->lag, from = c->cur ^ 1;
    const Route route = unit_route(c->plan, k, true);
    HipDev dev{c};
    int rc = c->order.one_stream(dev);   // (everything below runs on s_compute)
    if (rc) return rc;
    if (route == Route::one_launch) {
        rc = launch_deep(c, from, LAT_LAG, c->s_compute, k, true);
    } else if (route != Route::single_steps) {   // the frame, then the bulk (a slab: from the deep halo still in lat[from]'s ghost rows)
        // one row more than a launch unit computes (extra = 1): the field export pulls the slab's first / last row from the first
        // ghost rows of this lattice (the unit received S = k + 1 rows per side: enough)
        rc = launch_frame_work(c, route, from, LAT_LAG, c->s_compute, k, 1);
        if (rc == LBM_OK) rc = launch_deep(c, from, LAT_LAG, c->s_compute, k);
    } else {                            // k single steps (a lone lattice), through scratch lattice 2
        if (is_slab(c->plan)) return fail(c, LBM_ERR_STATE, "internal: the last unit of a slab cannot be replayed");
        if (k > 1 && (rc = ensure_scratch(c, 2)) != LBM_OK) return rc;
        int f = from;
        for (int i = 1; i <= k; ++i) {
            const int to = i == k ? LAT_LAG : (f == 2 ? 3 : 2);
            c->raw[to] = 0;
            rc = launch_rows(c, f, to, 0, 1, c->plan.geo.ny, c->s_compute);
            if (rc) return rc;
            f = to;
        }
    }
    if (rc) return rc;
    c->raw[LAT_LAG] = 0;
    c->lag_valid = true;
    return LBM_OK;
}

// One step of the push scheme: collide-and-push lat[cur] -> ftemp (lat[2]); wall rules on ftemp + copy -> lat[cur ^ 1].
int push_step(lbm_ctx* c) {
    const int rc = launch_variant(c, [&](auto v) {
        using VT = decltype(v);
        using R = typename VT::R;
        const dim3 g = grid_rows(c, c->plan.geo.ny);
        if constexpr (!sem_is_bb(VT::SEM)) {   // (validate_params refuses the push scheme with bounce-back walls)
            hipLaunchKernelGGL((k_push_collide<R, VT::COLL, VT::SEM>), g, dim3(BLK), 0, c->s_compute, c->lat[c->cur].as<const R>(), c->lat[2].as<R>(), c->plan.geo,
                               relax_of<R>(c->p));
            hipLaunchKernelGGL((k_push_bc<R, VT::COLL, VT::SEM>), g, dim3(BLK), 0, c->s_compute, c->lat[c->cur].as<const R>(), c->lat[2].as<R>(),
                               c->lat[c->cur ^ 1].as<R>(), c->plan.geo, (R)c->p.uLB);
        }
    });
    if (rc) return rc;
    finish_unit(c, 1);
    return LBM_OK;
}

// ftemp starts as a copy of fin (MRT_GPU.py:324)
int push_reset(lbm_ctx* c) {
    if (!c->plan.push) return LBM_OK;
    HIP_TRY(c, hipMemcpyAsync(c->lat[2].get(), c->lat[0].get(), (size_t)c->plan.bstride * c->plan.es, hipMemcpyDeviceToDevice, c->s_compute));
    return LBM_OK;
}

int step_many(lbm_ctx* c, int nsteps) {
    if (c->plan.push) {
        for (int i = 0; i < nsteps; ++i) {
            int rc = sample_if_due(c);
            if (rc == LBM_OK) rc = push_step(c);
            if (rc == LBM_OK) rc = sample_after_unit(c);
            if (rc) return rc;
        }
        return LBM_OK;
    }
    const bool slab = is_slab(c->plan);
    if (slab && !own_transport(c))
        return fail(c, LBM_ERR_STATE, "lbm_step on a slab without a communicator: its ghost rows would never be exchanged (attach one with "
                                      "lbm_comm_init, or drive the slab with lbm_step_edges/interior/finish, lbm_step_unit and the lbm_halo_* calls)");
    bool comm_used = false;
    HipDev dev{c};
    int rc = c->order.begin_call(dev, c->plan.kern != Kern::none || slab);   // (a lone lattice stepping one step per launch uses one stream, no events)
    if (rc) return rc;
    int left = nsteps;
    while (left > 0) {
        rc = sample_if_due(c);
        if (rc) return rc;
        const int S = unit_steps(c->plan, (int)steps_to_cut(c->sampler, c->nsteps, left), c->raw[c->cur] != 0, own_transport(c));
        rc = run_unit(c, &comm_used, S, true);
        if (rc == LBM_OK) rc = sample_after_unit(c);
        if (rc) return rc;
        left -= S;
    }
    if (slab && nsteps > 0 && !c->raw[c->cur]) {   // the populations lbm_get_fields returns for the slab's first / last row need the one-row halo
        rc = c->order.before_exchange(dev, 1);
        if (rc == LBM_OK) rc = enqueue_exchange(c, c->cur);
        if (rc) return rc;
        c->order.set_thin_valid(true);
        comm_used = true;
    }
    return comm_used ? c->order.end_call(dev) : LBM_OK;
}
}  // namespace lbmhost

using namespace lbmhost;

extern "C" {

int lbm_step(lbm_ctx* c, int nsteps) {
    if (!c || nsteps < 0) return fail(c, LBM_ERR_INVALID, "lbm_step: bad argument");
    HIP_TRY(c, hipSetDevice(c->p.device));
    return step_many(c, nsteps);
}

int lbm_time_steps(lbm_ctx* c, int nsteps, double* ms) {
    if (!c || nsteps < 0 || !ms) return fail(c, LBM_ERR_INVALID, "lbm_time_steps: bad argument");
    HIP_TRY(c, hipSetDevice(c->p.device));
    HIP_TRY(c, hipEventRecord(c->ev_t0, c->s_compute));
    int rc = step_many(c, nsteps);   // (joins the communication stream into s_compute before returning)
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_t1, c->s_compute));
    if (!spin_until_ready([&] { return hipEventQuery(c->ev_t1); })) HIP_TRY(c, hipEventSynchronize(c->ev_t1));
    float f = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&f, c->ev_t0, c->ev_t1));
    *ms = (double)f;
    return LBM_OK;
}

int lbm_step_edges(lbm_ctx* c) {
    if (!c) return LBM_ERR_INVALID;
    if (c->plan.push) return fail(c, LBM_ERR_STATE, "the split-step calls do not apply to kernel = PUSH");
    if (const char* stem = automatic_sampler(c->sampler))
        return fail(c, LBM_ERR_STATE, std::string("lbm_step_edges: automatic sampling (") + stem + "_begin, every > 0) runs inside lbm_step only");
    HIP_TRY(c, hipSetDevice(c->p.device));
    return launch_rows(c, c->cur, c->cur ^ 1, 0, c->plan.geo.ny - 1, 2, c->s_compute);
}

int lbm_step_interior(lbm_ctx* c) {
    if (!c) return LBM_ERR_INVALID;
    if (c->plan.push) return fail(c, LBM_ERR_STATE, "the split-step calls do not apply to kernel = PUSH");
    HIP_TRY(c, hipSetDevice(c->p.device));
    return launch_rows(c, c->cur, c->cur ^ 1, 1, 1, c->plan.geo.ny - 2, c->s_compute);
}

int lbm_step_finish(lbm_ctx* c) {
    if (!c) return LBM_ERR_INVALID;
    if (c->plan.push) return fail(c, LBM_ERR_STATE, "the split-step calls do not apply to kernel = PUSH");
    HIP_TRY(c, hipSetDevice(c->p.device));
    const int rc = periodic_wrap(c, c->cur ^ 1, c->s_compute);   // (periodic sides: the image cells of the lattice the two calls wrote)
    if (rc) return rc;
    finish_unit(c, 1);
    return c->scalar.active ? scalar_step(c) : LBM_OK;
}

int lbm_step_unit(lbm_ctx* c, int S) {
    if (!c) return LBM_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->p.device));
    if (c->plan.push || c->plan.kern == Kern::none) return fail(c, LBM_ERR_STATE, "lbm_step_unit: this context steps one step per launch (lbm_next_unit() is 1)");
    if (own_transport(c)) return fail(c, LBM_ERR_STATE, "lbm_step_unit: a communicator is attached, lbm_step() moves the halos itself");
    if (const char* stem = automatic_sampler(c->sampler))
        return fail(c, LBM_ERR_STATE, std::string("lbm_step_unit: automatic sampling (") + stem + "_begin, every > 0) runs inside lbm_step only");
    if (c->raw[c->cur]) return fail(c, LBM_ERR_STATE, "lbm_step_unit: the first step after an upload is a single step");
    const bool ok = c->plan.tb_steps == 2 ? S == 2 : (S >= 3 && S <= c->plan.tb_steps);
    if (!ok)
        return fail(c, LBM_ERR_INVALID, c->plan.tb_steps == 2 ? std::string("lbm_step_unit: this context runs units of 2 steps")
                                                         : "lbm_step_unit: unit_steps must be 3 .. " + std::to_string(c->plan.tb_steps) +
                                                               " (this context's steps per launch; lbm_next_unit plans 4 or more on a slab)");
    if (is_slab(c->plan) && !c->plan.deep_halo) return fail(c, LBM_ERR_STATE, "lbm_step_unit on a slab needs the deep halo (MRT_GPU semantics)");
    bool comm_used = false;
    HipDev dev{c};
    int rc = c->order.begin_call(dev, true);   // (INT covers the imported rows)
    if (rc == LBM_OK) rc = run_unit(c, &comm_used, S, false);
    if (rc) return rc;
    return comm_used ? c->order.end_call(dev) : LBM_OK;
}
}  // extern "C"
