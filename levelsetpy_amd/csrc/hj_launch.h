// What every launch of a tiled substep kernel shares, whatever the Hamiltonian type: the chunk plan of the launch (second
// plane range, edge ranges of a gated slab launch), the FusedArgs block, and the LAUNCH LAYER of the built-in kernels -- stage
// class, occupancy, plan record, dynamic-LDS grant, enqueue, timing dump.  Used by the instantiations of hj_inst.hip / hj_instx.hip
// (built-in Hamiltonians) and, for the plan and the arguments, by hj_rtc.hip (Hamiltonians compiled at run time with hipRTC).
#pragma once
#include <mutex>
#include "hj_host.h"
#include "hj_fused.h"

namespace hjh {

// MODE of the tiled kernels: plain RK stages (no clamp, no post-step operator, not ydot-only) run the flag-free instantiations -- 1 the
// Euler stage, 2 the stages that blend with y0 -- and 0 carries every run-time flag.  (honour_no_plain = false: callers that never
// read HJ_NO_PLAIN, hj_rtc.hip)
inline int stage_mode(const hj_ctx* c, const SubstepCall& s, bool honour_no_plain = true) {
    const bool plain = s.stage != HJ_STAGE_YDOT && s.restrict_sign == 0 && s.post_op == 0 && !(honour_no_plain && c->no_plain);
    return plain ? (s.stage == HJ_STAGE_EULER ? 1 : 2) : 0;
}

// Resident workgroups per CU of (kernel, dynamic LDS bytes) on the context's device, asked once per context.  Planning without a device
// estimates: the launch bound's waves per SIMD (occ_hint), and the CU's 160 KB of LDS -- and a planning look from a live context
// (c->dry == 2) must not cache its estimate: it is not the device's answer.
inline int wg_per_cu(hj_ctx* c, const void* kern, int nt, size_t lds_bytes, int occ_hint) {
    const auto key = std::make_pair(kern, lds_bytes);
    auto it = c->occ_cache.find(key);
    if (it != c->occ_cache.end()) return it->second;
    int nb = 0;
    if (c->dry) nb = std::max(1, std::min(occ_hint * 256 / nt, (int)((size_t)(160 * 1024) / std::max<size_t>(1, lds_bytes))));
    else if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, nt, lds_bytes) != hipSuccess || nb < 1) nb = 1;
    if (c->dry != 2) c->occ_cache.emplace(key, nb);
    return nb;
}

// What hj_last_kernel / hj_last_tile / hj_launch_record report of a launch: chunk length and tile extents (E null: a kernel without tiles)
inline void record_launch(hj_ctx* c, const char* name, const void* kern, int chunk = 0, const int* E = nullptr, int nd = 0) {
    c->last_kernel = name;
    c->note_kernel(kern);
    c->last_E[0] = chunk;
    for (int d = 1; d < HJ_MAX_DIM; ++d) c->last_E[d] = (E && d < nd) ? E[d] : 0;
}
// ... and what hj_plan_substep reports of a tiled launch; a dry context returns right after this
inline void record_plan(hj_ctx* c, const Tiling& t, int nt, int occ_blocks, const char* name, const void* kern, int nd) {
    c->last_plan.ntiles = t.ntiles; c->last_plan.nchunks = t.nchunks; c->last_plan.nblocks = t.nblocks; c->last_plan.threads = nt;
    c->last_plan.wg_per_cu = occ_blocks; c->last_plan.lds_bytes = t.lds_bytes;
    record_launch(c, name, kern, t.chunk, t.E, nd);
}

// More than 64 KB of dynamic LDS has to be granted to the function: once per (device, kernel), raised but never lowered -- the attribute
// belongs to the function, not to a context.  One table for the whole library (an inline function's statics are shared by its objects).
inline int grant_dynamic_lds(const hj_ctx* c, const void* kern, size_t lds_bytes) {
    if (lds_bytes <= 64 * 1024) return HJ_OK;
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> granted_by_kernel;
    std::lock_guard<std::mutex> lock(mu);
    size_t& granted = granted_by_kernel[std::make_pair(c->device, kern)];
    if (granted < lds_bytes) {
        HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        granted = lds_bytes;
    }
    return HJ_OK;
}

// The launch of a tiled substep kernel (y, y0, out, FusedArgs) on the call's stream, its LDS granted first
template <typename K, typename T, int ND>
int enqueue(hj_ctx* c, const SubstepCall& s, K kern, unsigned grid_blocks, int nt, size_t lds_bytes, const FusedArgs<T, ND>& A) {
    const int rc = grant_dynamic_lds(c, reinterpret_cast<const void*>(kern), lds_bytes);
    if (rc) return rc;
    if (c->launch_stop) {
        // completion signal attached to the dispatch packet itself: a separate hipEventRecord costs a
        // marker packet and ~6 us of bubble before the next kernel of the stream (slab timeline)
        hipExtLaunchKernelGGL(kern, dim3(grid_blocks), dim3(nt), (unsigned)lds_bytes, call_stream(c, s), nullptr, c->launch_stop, 0,
                              (const T*)s.y, (const T*)s.y0, (T*)s.out, A);
        c->launch_stop = nullptr;
    } else {
        hipLaunchKernelGGL(kern, dim3(grid_blocks), dim3(nt), lds_bytes, call_stream(c, s), (const T*)s.y, (const T*)s.y0, (T*)s.out, A);
    }
    HIP_TRY(hipGetLastError());
    return HJ_OK;
}

// HJ_TIMING_DUMP (read at ctx creation): per-workgroup start/end clocks of every launch.  timing_begin hands the launch its buffer
// (FusedArgs::timing; null: no dump asked for), timing_end waits for the launch and appends its rows to the file
// (tools/block_timing.py, tools/stamp_summary.py).
inline int timing_begin(hj_ctx* c, const SubstepCall& s, int nblocks, unsigned long long*& tbuf) {
    tbuf = nullptr;
    if (!(c->timing_dump && *c->timing_dump)) return HJ_OK;
    HIP_TRY(hipMalloc(&tbuf, (size_t)nblocks * 12 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(tbuf, 0, (size_t)nblocks * 12 * sizeof(unsigned long long), call_stream(c, s)));
    return HJ_OK;
}
inline int timing_end(hj_ctx* c, const SubstepCall& s, const Tiling& t, unsigned long long* tbuf) {
    if (!tbuf) return HJ_OK;
    std::vector<unsigned long long> h((size_t)t.nblocks * 12);
    HIP_TRY(hipStreamSynchronize(call_stream(c, s)));
    HIP_TRY(hipMemcpy(h.data(), tbuf, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipFree(tbuf));
    if (FILE* f = fopen(c->timing_dump, "a")) {
        fprintf(f, "# launch nblocks=%d ntiles=%d chunk=%d stage=%d\n", t.nblocks, t.ntiles, t.chunk, s.stage);
        for (int i = 0; i < t.nblocks; ++i) {
            fprintf(f, "%d %llu %llu %llu %llu", i, h[4 * i], h[4 * i + 1], h[4 * i + 2], h[4 * i + 3]);
            // HJ_STAMP builds: shader-clock sums of the four phases of wave 0 and of the last wave (else zeros)
            const unsigned long long* ph = h.data() + 4 * (size_t)t.nblocks + 8 * (size_t)i;
            fprintf(f, " %llu %llu %llu %llu %llu %llu %llu %llu\n", ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[6], ph[7]);
        }
        fclose(f);
    }
    return HJ_OK;
}

struct EdgePlan { int echunk = 0, ne[2] = {0, 0}, edge_count = 0; };

// chunk_max > 0: no chunk longer than this many planes (kernels whose LDS use grows with the chunk: hj_fused4v.h)
inline int plan_chunks(hj_ctx* c, const SubstepCall& s, Tiling& t, int occ_blocks, EdgePlan& ep, int64_t chunk_max = 0) {
        choose_chunks(c, t, s.p0, s.p1, occ_blocks, chunk_max);
        if (!t.ok) return hjh::fail(HJ_EUNSUPPORTED, "axis-0 plane too large for the tiled kernel");
        t.nchunks1 = t.nchunks;
        if (s.q1 > s.q0) {     // second range: same chunk length
            t.nchunks += (int)((s.q1 - s.q0 + t.chunk - 1) / t.chunk);
            t.nblocks = t.nchunks * t.ntiles;
            t.bpx = (t.nblocks + 7) / 8;
        }
        if (s.gated) {
            // edge chunks of HJ_STENCIL planes each, ahead of everything else (hj_fused.h: logical_block, chunk_planes)
            ep.echunk = HJ_STENCIL;
            for (int w = 0; w < 2; ++w) ep.ne[w] = (int)((s.e1[w] - s.e0[w] + ep.echunk - 1) / ep.echunk);
            const int main_blocks = t.nblocks;
            ep.edge_count = (ep.ne[0] + ep.ne[1]) * t.ntiles;
            t.nblocks = main_blocks + ep.edge_count;
            t.bpx = (main_blocks + 7) / 8;
        }
    return HJ_OK;
}

// everything of FusedArgs but the intended WENO5's epsilon fields (eps_part / eps_rows) and the debug timing buffer
template <typename T, int ND>
int fill_fused_args(hj_ctx* c, const SubstepCall& s, const Tiling& t, const EdgePlan& ep, int scheme, bool pair,
                    FusedArgs<T, ND>& A, unsigned& grid_blocks) {
    long long st = 1;
    for (int d = ND - 1; d >= 0; --d) {
        A.inv_dx[d] = (T)(1.0 / c->dx[d]);
        A.n[d] = (int)c->N[d];
        A.bc[d] = c->bc[d];
        A.km[d] = c->tz[d] ? T(-1) : T(1);
        fill_stencil_constants<T>(c->dx[d], A.K[d]);
        A.sc[d] = scheme_scale<T>(scheme, c->dx[d]);
        A.pstride[d] = (d >= 1) ? (int)st : 0;
        if (d == 0) A.stride0 = st;
        st *= c->N[d];
        A.E[d] = t.E[d];
        A.ntile[d] = t.ntile[d];
    }
    for (int d = 0; d < ND; ++d) A.tb[d] = 0;
    if constexpr (ND == 4) { if (c->tile_block[0] > 0 && c->tile_block[1] > 0) { A.tb[1] = c->tile_block[0]; A.tb[2] = c->tile_block[1]; } }
    A.halo_lo = c->halo_lo;
    A.halo_hi = c->halo_hi;
    A.ntiles = t.ntiles;
    A.lpitch = t.lpitch;
    A.chunk = t.chunk;
    A.nchunks = t.nchunks;
    A.plane_begin = (int)s.p0;
    A.plane_end = (int)s.p1;
    A.plane_begin2 = (int)s.q0;
    A.plane_end2 = (int)s.q1;
    A.nchunks1 = t.nchunks1;
    A.nblocks = t.nblocks;
    if (t.nblocks >= (1 << 22)) return hjh::fail(HJ_EUNSUPPORTED, "more than 4 M workgroups in one launch (index arithmetic of the kernels)");
    A.blocks_per_xcd = t.bpx;
    // chunks marching pairwise in opposite directions (pair kernel; only in -DHJ_MAYDOWN=1 builds, hj_fused.h): not with edge ranges or a
    // second range in the launch
    A.npairs = (HJ_MAYDOWN && pair && c->pair_dirs && !s.gated && s.q1 <= s.q0 && ep.edge_count == 0) ? t.nchunks1 / 2 : 0;
    A.echunk = ep.echunk;
    A.nchunks_e1 = ep.ne[0];
    A.nchunks_e = ep.ne[0] + ep.ne[1];
    for (int w = 0; w < 2; ++w) { A.eplane[w][0] = (int)s.e0[w]; A.eplane[w][1] = (int)s.e1[w]; }
    A.edge_count = ep.edge_count;
    A.edge_bpx = (ep.edge_count + 7) / 8;
    A.edge_blocks = 8 * A.edge_bpx;
    A.gate = (s.gated && ep.edge_count > 0) ? c->gate : nullptr;
    c->gate_posted = A.gate ? ep.edge_count : 0;
    grid_blocks = (unsigned)(A.edge_blocks + t.bpx * 8);
    A.lds_nbuf = pair ? c->last_nbuf : 2;
    A.halo_ahead = (pair && c->last_nbuf > 2) ? c->last_nbuf - 2 : 0;
    A.stage = s.stage;
    A.ydot_only = (s.stage == HJ_STAGE_YDOT);
    A.use_y0 = (s.stage >= HJ_STAGE_RK3_HALF);
    switch (s.stage) {                          // out = ca*y0 + cb*(y + dt*ydot)
        case HJ_STAGE_RK3_HALF: A.ca = T(0.75); A.cb = T(0.25); break;           // ode_cfl_3.py:184,193
        case HJ_STAGE_RK3_FULL: A.ca = T(1.0 / 3.0); A.cb = T(2.0 / 3.0); break; // :226,241
        case HJ_STAGE_RK2_FULL: A.ca = T(0.5); A.cb = T(0.5); break;             // ode_cfl_2.py:184,201
        default: A.ca = T(0); A.cb = T(1); break;
    }
    A.dt = (T)s.dt;
    A.dt_dev = s.dt_dev;
    A.post_op = s.post_op;
    A.do_clamp = s.restrict_sign != 0;
    A.clamp_lo = s.restrict_sign > 0 ? T(0) : -std::numeric_limits<T>::infinity();
    A.clamp_hi = s.restrict_sign < 0 ? T(0) : std::numeric_limits<T>::infinity();
    fill_ham<T>(c, s.par, A.ham, s.ham);
    if (s.term) {            // a TermOp launch: coefficient array 0 rides in the y0 stream whatever the stage says
        A.term = *static_cast<const hj::TermPar<T>*>(s.term);
        A.use_y0 = A.term.arr[0] != nullptr;
        for (int d = 0; d < ND; ++d) A.sc[d] = T(1);
    }
    return HJ_OK;
}

}  // namespace hjh
