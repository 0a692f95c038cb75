// pt_hip.hip — gfx950 kernels + C-ABI (include/pt_capi.h) of the MI355X path
// tracer.  Replaces the reference's spp x bounce loop (main.py:186-280) and its
// two Pool callables (intersect_objects main.py:83, compute_color main.py:142).
//
// Kernel geometry: one work-item per (pixel, sample-slice);
// `split` adjacent lanes share a pixel and stride its samples, so the whole
// pixel lives in one wave and is reduced with DPP/shuffles in a fixed order
// (deterministic).  Triangles are read with uniform indices -> scalar loads
// (s_load_dwordx16) from the 80-B f32 filter records; only rare ambiguous
// tests touch the f64 records.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "pt_path.h"
#include "pt_wavefront.h"
#include "pt_prepare.h"
#include "pt_image.h"
#include "pt_ingest.h"
#include "pt_denoise.h"

using namespace pt;

// ------------------------------------------------------------- errors --
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define RCCHK(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)   // a callee's error is ours
#define HIPCHK(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess)                                                     \
            return fail(PT_EHIP, std::string(#expr " failed: ") + hipGetErrorString(e_)); \
    } while (0)

// ------------------------------------------------------------- kernels --
// k_render and its launch records: pt_render.h
#include "pt_render.h"
#include "pt_plan.h"   // the launch rules, without the HIP runtime
#include "pt_aa.h"   // the antialiasing kernels' launchers (pt_aa.hip)
#include "pt_lens.h" // the thin-lens kernels' launchers (pt_lens.hip)
#include "pt_rays.h" // the ray kernel's launcher (pt_rays.hip)
#include "pt_rays_list.h" // a ray accumulator's kernels' launchers (pt_rays_list.hip)
#if PT_K2_OWN_TU
extern template __global__ void k_render<false, false, false>(SceneK, RenderK, void*, StatsDev*);
#endif

// ------------------------------------------------- wavefront (BVH scenes) --
// the list appends' helpers and the shade kernels (pt_shade.hip): pt_shade.h
#include "pt_shade.h"

// The shadow walks' query list is sorted by the origin's cell (wf_cell, 12
// Morton bits) before each walk step (render_wavefront): lanes of a wave then
// walk from nearby origins toward the light, and the shadow walks run 10%
// faster.  The closest list stays unsorted (random
// directions: its walks did not gain).
// The sort: a counting sort on the 12-bit cell key without the host — the
// list's length n is read on the device.  nb = bin_cols(n)
// blocks (at most kBinBlocks, at least kBinMinChunk entries each, so a short
// list pays a small count matrix) each take a contiguous chunk of the list;
// k_bin_hist counts its keys per cell (LDS) into the cell-major count matrix
// (kBins x nb), k_bin_rows turns each cell's row into its exclusive prefix
// sums in place (one wave per row) and writes the row's total, k_bin_base
// scans the kBins totals (one block), and k_bin_scatter places the chunk's
// entries at base[cell] + row prefix (LDS cursors): every entry lands exactly
// once, in (cell, block, position-in-block) order.  Hand-written two-level
// scan, no decoupled lookback: a lookback scan's blocks can wait behind the
// persistent closest-walk blocks that share the GPU (DESIGN.md §11, 13.7 ms
// per call for hipCUB's).
constexpr int kBinBits = 12, kBins = 1 << kBinBits, kBinBlocks = 1024, kBinMinChunk = 2048;
static_assert(kBinBlocks <= 64 * 16, "k_bin_rows: a row is at most 16 entries per lane");
static_assert(kBins % 4 == 0 && kBins == 4 * 1024, "k_bin_rows: 4 rows per block; k_bin_base: 4 per thread");
__device__ __forceinline__ int32_t bin_cols(int32_t n) {
    const int32_t c = (n + kBinMinChunk - 1) / kBinMinChunk;
    return c < 1 ? 1 : (c > kBinBlocks ? kBinBlocks : c);
}
__device__ __forceinline__ void bin_chunk(int32_t n, int32_t nb, int32_t* b0, int32_t* b1) {
    const int32_t chunk = (n + nb - 1) / nb;
    *b0 = min(n, (int32_t)blockIdx.x * chunk);
    *b1 = min(n, *b0 + chunk);
}
// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}
__global__ __launch_bounds__(256) void k_bin_hist(const uint16_t* __restrict__ keys, const int32_t* count,
                                                  uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kBins];
    const int32_t n = *count, nb = bin_cols(n);
    if ((int32_t)blockIdx.x >= nb) return;   // (block-uniform, before any barrier)
    for (int i = threadIdx.x; i < kBins; i += 256) h[i] = 0u;
    __syncthreads();
    int32_t b0, b1;
    bin_chunk(n, nb, &b0, &b1);
    for (int32_t i = b0 + (int32_t)threadIdx.x; i < b1; i += 256) atomicAdd(&h[keys[i] & (kBins - 1)], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < kBins; i += 256) hist[(size_t)i * nb + blockIdx.x] = h[i];
}
// kBins / 4 blocks: one row of the count matrix per wave, lane l holding the
// row's entries [l per, (l + 1) per); the row becomes its exclusive prefix
// sums, its total goes to rowsum
__global__ __launch_bounds__(256) void k_bin_rows(uint32_t* __restrict__ hist, const int32_t* count,
                                                  uint32_t* __restrict__ rowsum) {
    const int32_t nb = bin_cols(*count);
    const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    uint32_t* r = hist + (size_t)row * nb;
    const int per = (nb + 63) >> 6;
    uint32_t v[16], s = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = lane * per + j;
        v[j] = (j < per && i < nb) ? r[i] : 0u;
        s += v[j];
    }
    const uint32_t incl = wave_incl_scan(s);
    uint32_t x = incl - s;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = lane * per + j;
        if (j < per && i < nb) r[i] = x;
        x += v[j];
    }
    if (lane == 63) rowsum[row] = incl;
}
// one block of 1024: the exclusive prefix sums of the kBins row totals
__global__ __launch_bounds__(1024) void k_bin_base(const uint32_t* __restrict__ rowsum,
                                                   uint32_t* __restrict__ base) {
    __shared__ uint32_t wsum[16];
    const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t v[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = rowsum[4 * t + j]; s += v[j]; }
    const uint32_t incl = wave_incl_scan(s);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t x = incl - s;
    for (int i = 0; i < w; ++i) x += wsum[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) { base[4 * t + j] = x; x += v[j]; }
}
__global__ __launch_bounds__(256) void k_bin_scatter(const uint16_t* __restrict__ keys,
                                                     const int32_t* __restrict__ vals, const int32_t* count,
                                                     const uint32_t* __restrict__ off,
                                                     const uint32_t* __restrict__ base,
                                                     int32_t* __restrict__ out) {
    __shared__ uint32_t cur[kBins];
    const int32_t n = *count, nb = bin_cols(n);
    if ((int32_t)blockIdx.x >= nb) return;   // (block-uniform, before any barrier)
    for (int i = threadIdx.x; i < kBins; i += 256) cur[i] = base[i] + off[(size_t)i * nb + blockIdx.x];
    __syncthreads();
    int32_t b0, b1;
    bin_chunk(n, nb, &b0, &b1);
    for (int32_t i = b0 + (int32_t)threadIdx.x; i < b1; i += 256)
        out[atomicAdd(&cur[keys[i] & (kBins - 1)], 1u)] = vals[i];
}

// Next list positions for the lanes that need one.  A wave claims a chunk of
// kWfChunk consecutive positions with one atomic on the list head and hands
// them out to its lanes as they need work; it claims the next chunk only when
// this one runs out (one global atomic per ~kWfChunk queries instead of one
// per refill turn).  [cb, ce): the wave's unclaimed rest (wave-uniform).
#ifndef PT_WF_CHUNK
#define PT_WF_CHUNK 64
#endif
constexpr int32_t kWfChunk = PT_WF_CHUNK;
static_assert(kWfChunk >= 64, "a refill turn can need a position for every lane of a wave");
__device__ __forceinline__ int32_t wf_fetch(bool need, int32_t* head, int32_t& cb, int32_t& ce) {
    const uint64_t m = __ballot(need);
    const int32_t n = (int32_t)__popcll(m);
    const int32_t idx = (int32_t)lanes_below(m);   // rank among the needing lanes
    const int32_t avail = ce - cb;
    int32_t pos = cb + idx;
    if (n > avail) {   // wave-uniform: claim the next chunk
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
        int32_t base = 0;
        if (lane_id() == leader) base = atomicAdd(head, kWfChunk);
        base = __shfl(base, (int)leader);
        if (idx >= avail) pos = base + (idx - avail);
        cb = base + (n - avail);
        ce = base + kWfChunk;
    } else {
        cb += n;
    }
    return pos;
}

// The primary rays: one work-item per pixel (a pixel's `split` slots share
// it, main.py:191): the uniform part of the eye ray into CQP[pixel], whose
// BVH part is a closest query (list entry = pixel; spill home = the pixel's
// first slot).  Every slot of the pixel finishes it in its first shade step.
__global__ __launch_bounds__(256) void k_wf_primary(SceneK S, RenderK R, WfPath* __restrict__ W,
                                                    WfClosestQ* __restrict__ CQP,
                                                    int32_t* __restrict__ list, int32_t* counters) {
    const uint32_t pix = blockIdx.x * 256u + threadIdx.x;
    const uint32_t want = wf_primary_step(S, WfFrame{R}, pix, W, CQP);
    wf_append((want & kWfWantClosest) != 0, counters, list, (int32_t)pix);
}
// Persistent walk kernels over the 4-wide quantised BVH (QNode): a
// work-item holds one query at a time and takes the next one from the list
// as soon as its walk ends.  A loop turn is one
// "while-while" round, except that the node phase ends for the whole wave
// once at most `thr` of its lanes are still descending and some lane has a
// leaf to test (the others carry on in the next turn): the wave does not wait
// for its longest node run, and lanes whose walk ended are refilled every
// turn.  Every turn makes progress (a node step, a leaf or a fetch), and a
// lane whose list is exhausted stays idle, so the loop drains.
// Walk stacks: kWalkStack entries per work-item, the first kWalkStackLds in
// shared memory (the top of a stack, where nearly all pushes and pops land),
// the rest in global memory.  Smaller shared-memory stacks let more
// work-groups share a CU (the walks wait on dependent node loads: occupancy
// is their latency hiding).
#ifndef PT_SHADOW_WAVES   // one-ray shadow walk: 5 waves/SIMD (90 VGPRs, no spills; 6: spills)
#define PT_SHADOW_WAVES 5
#endif
#ifndef PT_CLOSEST_WAVES
#define PT_CLOSEST_WAVES 5
#endif
#ifndef PT_WALK_STACK_LDS
#define PT_WALK_STACK_LDS 16
#endif
constexpr int kWalkStack = 48;                   // entries of a walk kernel's stack (= kBvhStack)
constexpr int kWalkStackLds = PT_WALK_STACK_LDS;  // of them in shared memory
constexpr int kWalkStackGlobal = kWalkStack - kWalkStackLds;
// COUNT (PT_FLAG_WALK_COUNT launches only): per-query work of the walk —
// queries, 4-wide node visits, leaf-unit tests — summed into wc[0..2]
// (the walks' algorithmic bytes).
template <bool COUNT>
__device__ __forceinline__ void flush_walk_counts(uint32_t q, uint32_t nodes, uint32_t units,
                                                  unsigned long long* wc) {
    if (!COUNT) return;
    uint32_t v[3] = {q, nodes, units};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        uint32_t x = v[i];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
        if ((threadIdx.x & 63) == 0 && x) atomicAdd(&wc[i], (unsigned long long)x);
    }
}
__device__ __forceinline__ uint32_t leaf_units(int ref) { return (uint32_t)(~ref) & 7u; }

// The shadow walks: one work-item per open shadow ray (list entries
// (slot << 2) | ray, pt_path.h "one-ray shadow walks").
template <bool UC, bool COUNT>
__global__ __launch_bounds__(256, PT_SHADOW_WAVES) void k_wf_shadow(SceneK S, WfPath* __restrict__ W,
                                                   WfShadowQ* __restrict__ SQ,
                                                   const int32_t* __restrict__ list, int32_t* counters,
                                                   int32_t thr, unsigned long long* wc,
                                                   int* __restrict__ ovf) {
    uint32_t c_q = 0, c_nodes = 0, c_units = 0;
    const int32_t count = counters[0];
    int32_t cb = 0, ce = 0;   // this wave's claimed list positions (wf_fetch)
    int32_t slot = -1;
    bool exhausted = false;
    // the walk stack: its top kWalkStackLds entries in shared memory
    // (4 B each per lane), the rest in global memory
    __shared__ int stack[kWalkStackLds][256];
    const int lanes = (int)gridDim.x * 256, gl = (int)(blockIdx.x * 256u + threadIdx.x);
    const ShadowStackLds K{(PT_LDS int*)&stack[0][threadIdx.x], 256, ovf + gl, lanes, kWalkStackLds};
    Shadow1 r;
    ShadowTrav1 T;
    T.ref = kNoRef;
    int pl = kNoRef, pl2 = kNoRef;   // postponed leaves
    while (true) {
        const bool need = slot < 0 && !exhausted;
        if (__any(need)) {
            const int32_t i = wf_fetch(need, &counters[1], cb, ce);
            if (need) {
                if (i < count) {
                    const int32_t e = list[i];
                    slot = e >> 2;
                    if (COUNT) ++c_q;
                    F3 o32;
                    int ogrp;
                    wf_get_shadow1(SQ[slot], e & 3, &o32, &ogrp, &r);
                    s1_init(T, S, o32, ogrp, r, S.qroot);
                } else {
                    exhausted = true;
                }
            }
        }
        if (__all(slot < 0)) break;
        // node phase (wave-uniform loop).  Speculative: a lane that reaches a
        // leaf postpones it (pl) and keeps walking, so a turn can test two
        // leaves per lane and fewer lanes idle in this loop.
        while (true) {
            if (slot >= 0 && T.ref <= -2 && pl2 == kNoRef) {
                if (pl == kNoRef) pl = T.ref;
                else pl2 = T.ref;
                T.ref = s1_pop(T, K, S, r);
            }
            const bool desc = slot >= 0 && T.ref >= 0;
            const int32_t nd = (int32_t)__popcll(__ballot(desc));
            // end it early only when some lane has a leaf to test (progress)
            if (nd == 0 || (nd <= thr && __any(slot >= 0 && (pl != kNoRef || T.ref <= -2)))) break;
            if (desc) {
                if (COUNT) ++c_nodes;
                s1_qnode(T, K, S, r);
            }
        }
        if (slot >= 0) {
            const Spill sp{W[slot].sp, 1};
            if (COUNT)
                c_units += (pl != kNoRef ? leaf_units(pl) : 0u) + (pl2 != kNoRef ? leaf_units(pl2) : 0u) +
                           (T.ref <= -2 ? leaf_units(T.ref) : 0u);
            if (pl != kNoRef) s1_units<UC, PT_WF_LRNG != 0>(T, S, &r, sp, pl);
            if (pl2 != kNoRef) s1_units<UC, PT_WF_LRNG != 0>(T, S, &r, sp, pl2);
            pl = pl2 = kNoRef;
            if (T.ref <= -2) {
                s1_units<UC, PT_WF_LRNG != 0>(T, S, &r, sp, T.ref);
                T.ref = s1_pop(T, K, S, r);
            }
            // a ray closed meanwhile drops what is left (entries, a node)
            if (!shadow1_open(S, r)) T.ref = kNoRef;
        }
        if (slot >= 0 && T.ref == kNoRef) {
            wf_put_shadow1(&SQ[slot], r);
            slot = -1;
        }
    }
    flush_walk_counts<COUNT>(c_q, c_nodes, c_units, wc);
}

template <bool UC, bool COUNT>
__global__ __launch_bounds__(256, PT_CLOSEST_WAVES) void k_wf_closest(SceneK S, WfPath* __restrict__ W,
                                                    WfClosestQ* __restrict__ CQ,
                                                    const int32_t* __restrict__ list, int32_t* counters,
                                                    int32_t thr, unsigned long long* wc,
                                                    int* __restrict__ ovf_ref,
                                                    uint16_t* __restrict__ ovf_dist,
                                                    uint32_t wshift) {
    // wshift: list entries index CQ; the spill home of entry e is
    // W[e << wshift] (the primary queries: one per pixel, its first slot's home)
    uint32_t c_q = 0, c_nodes = 0, c_units = 0;
    const int32_t count = counters[0];   // [count, head]
    int32_t cb = 0, ce = 0;   // this wave's claimed list positions (wf_fetch)
    int32_t slot = -1;
    bool exhausted = false;
    ClosestAcc ca = closest_init();
    ClosestTrav T;
    // the walk stack: its top kWalkStackLds entries in shared memory (6 B
    // each per lane), the rest in global memory
    __shared__ int sref[kWalkStackLds][256];
    __shared__ uint16_t sdist[kWalkStackLds][256];
    const int lanes = (int)gridDim.x * 256, gl = (int)(blockIdx.x * 256u + threadIdx.x);
    const ClosestStackLds K{(PT_LDS int*)&sref[0][threadIdx.x], (PT_LDS uint16_t*)&sdist[0][threadIdx.x], 256,
                            ovf_ref + gl,
                         ovf_dist + gl, lanes, kWalkStackLds};
    T.ref = kNoRef;
    int pl = kNoRef, pl2 = kNoRef;   // postponed leaves
    while (true) {
        const bool need = slot < 0 && !exhausted;
        if (__any(need)) {
            const int32_t i = wf_fetch(need, &counters[1], cb, ce);
            if (need) {
                if (i < count) {
                    slot = list[i];
                    if (COUNT) ++c_q;
                    const WfClosestQ q = CQ[slot];
                    ca = wf_get_acc(q);
                    ctrav_init(T, S, F3{q.o[0], q.o[1], q.o[2]}, q.ogrp, F3{q.d[0], q.d[1], q.d[2]},
                               ca.b1, S.qroot);
                } else {
                    exhausted = true;
                }
            }
        }
        if (__all(slot < 0)) break;
        while (true) {   // node phase, speculative as in k_wf_shadow
            if (slot >= 0 && T.ref <= -2 && pl2 == kNoRef) {
                if (pl == kNoRef) pl = T.ref;
                else pl2 = T.ref;
                T.ref = ctrav_pop(T, K, ca.b1);
            }
            const bool desc = slot >= 0 && T.ref >= 0;
            const int32_t nd = (int32_t)__popcll(__ballot(desc));
            if (nd == 0 || (nd <= thr && __any(slot >= 0 && (pl != kNoRef || T.ref <= -2)))) break;
            if (desc) {
                if (COUNT) ++c_nodes;
                ctrav_qnode(T, K, S, &ca);
            }
        }
        if (slot >= 0) {
            const Spill sp{W[(size_t)slot << wshift].sp, 1};
            if (COUNT)
                c_units += (pl != kNoRef ? leaf_units(pl) : 0u) + (pl2 != kNoRef ? leaf_units(pl2) : 0u) +
                           (T.ref <= -2 ? leaf_units(T.ref) : 0u);
            if (pl != kNoRef) ctrav_units<false, UC>(T, S, &ca, sp, nullptr, pl);
            if (pl2 != kNoRef) ctrav_units<false, UC>(T, S, &ca, sp, nullptr, pl2);
            pl = pl2 = kNoRef;
            if (T.ref <= -2) ctrav_leaf<false, UC>(T, K, S, &ca, sp, nullptr);
        }
        if (slot >= 0 && T.ref == kNoRef) {
            CQ[slot].a1 = ca.a1;
            CQ[slot].a2 = ca.a2;
            CQ[slot].b1 = ca.b1;
            CQ[slot].i1 = ca.i1;
            slot = -1;
        }
    }
    flush_walk_counts<COUNT>(c_q, c_nodes, c_units, wc);
}

__global__ __launch_bounds__(256) void k_wf_final(SceneK S, RenderK R, const WfPath* __restrict__ W,
                                                  void* __restrict__ out) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    const SlotJob j = slot_job(S, R, tid);
    const D3 acc = j.valid ? ld3(W[tid].acc) : d3(0, 0, 0);
    store_pixel(R, j, acc, out, R.split);
}

// ------------------------------------ adaptive sampling (pt_accum) --
// Per-pixel moments S, Q and counts n on the device (include/pt_capi.h,
// pt_accum; the rule and the lane code: pt_path.h MomentSink, moment_err).
// A pass renders a LIST of pixels: k_accum_select_* build it (err, the active
// predicate, an ordered compaction), k_render_list adds k samples to each
// listed pixel, k_accum_resolve writes S / n as a framebuffer (ListK:
// pt_job.h).
// The lane's home of S and Q across the bounce loop: 0 the lane's registers
// (MomentRegs), 1 a device buffer [6][lanes], touched only when a path ends
// (MomentMem).  Both stay at 128 VGPRs / 64 B scratch; the registers are 5%
// faster on the K2 frame, the buffer stays as a tuning build.
#ifndef PT_MOMENT_HOME
#define PT_MOMENT_HOME 0
#endif
#ifndef PT_LIST_WAVES
#define PT_LIST_WAVES PT_RENDER_WAVES
#endif
// A work-item is (list entry, sample slice): `split` adjacent lanes share the
// entry's pixel e and stride the k samples its pass adds, from sample n[e] on.
// The pixel's lanes reduce S and Q in store_pixel's xor order and lane 0 adds
// them to the accumulator with plain loads and stores (the list is unique).
// (The four list kernels each write this reduce and commit out: as one
// helper, the sums by value, by reference, or with the store's condition
// inside it, every unit's code moved: this one -1024 B, pt_aa.hip -1688 B,
// pt_lens.hip +1340 B, pt_rays_list.hip +1280 B.)
template <bool FORCE64, bool BVH>
__global__ __launch_bounds__(kRenderBlock, PT_LIST_WAVES) void k_render_list(
    SceneK S, ListK R, const uint32_t* __restrict__ list, double* __restrict__ accS,
    double* __restrict__ accQ, uint32_t* __restrict__ accN, double* __restrict__ home) {
    __shared__ double spill[kSpillSlots][kRenderBlock];
    const Spill sp{&spill[0][threadIdx.x], (int)kRenderBlock};
    const uint32_t tid = blockIdx.x * kRenderBlock + threadIdx.x;
    const uint32_t entry = tid >> R.split_log2, c = tid & (R.split - 1u);
    // (entries that are no pixel of the frame are skipped, never dereferenced)
    const uint32_t e = entry < R.n_list ? list[entry] : 0xffffffffu;
    const bool valid = e < R.npix;   // the same for all lanes of an entry
#if PT_MOMENT_HOME
    MomentMem M{home + tid, (size_t)R.lanes};
#else
    MomentRegs M;
    (void)home;
#endif
    uint32_t k = 0;
    if (valid) {
        M.clear();
        const uint32_t n0 = accN[e];
        k = adapt_k(n0, R.A);
        const int32_t row = (int32_t)(e / (uint32_t)R.W);
        const int32_t ix = (int32_t)e - row * R.W, iy = R.H - 1 - row;
        const D3 eye = ld3(S.eye);
        const double x = linspace_at(S.ortho[0], S.ortho[2], R.W, ix);
        const double y = linspace_at(S.ortho[1], S.ortho[3], R.H, iy);
        const D3 d0 = d3(x - eye.x, y - eye.y, 0.0 - eye.z);
        LaneJob J;
        J.seed = R.seed;
        J.pixel = (uint32_t)ix * (uint32_t)R.H + (uint32_t)iy;
        J.sample0 = (int32_t)(n0 + c);
        J.sample_stride = (int32_t)R.split;
        J.n_samples = c < k ? (int32_t)((k - c + R.split - 1u) >> R.split_log2) : 0;
        J.bounces = R.bounces;
        J.rr_depth = R.rr_depth;
        Counters cnt = {};
        D3 P0 = d3(0, 0, 0);
        int tri0 = -1;
        // the primary hit once per lane and pass (k, like valid, is the same
        // in every lane of the entry: the whole group takes one branch)
        if (PT_PRIMARY_SHARED && !FORCE64 && !BVH && R.split >= PT_PRIMARY_SHARED) {
            if (R.bounces > 0 && k > 0) tri0 = primary_shared(S, eye, d0, c, R.split, sp, &P0);
        } else if (J.n_samples > 0 && R.bounces > 0) {
            tri0 = closest<FORCE64, false, BVH>(S, eye, d0, -1, sp, &P0, &cnt, true);
        }
        render_lane_cached<FORCE64, false, BVH>(S, J, FrameHit{tri0, d0}, P0, sp, &cnt, MomentSink<decltype(M)>{M});
    }
    D3 s = valid ? M.sum() : d3(0, 0, 0), q = valid ? M.sumsq() : d3(0, 0, 0);
    for (uint32_t m = 1; m < R.split; m <<= 1) {
        s.x += __shfl_xor(s.x, (int)m); s.y += __shfl_xor(s.y, (int)m); s.z += __shfl_xor(s.z, (int)m);
        q.x += __shfl_xor(q.x, (int)m); q.y += __shfl_xor(q.y, (int)m); q.z += __shfl_xor(q.z, (int)m);
    }
    if (valid && c == 0 && k > 0) {
        double* ps = accS + (size_t)e * 3;
        double* pq = accQ + (size_t)e * 3;
        ps[0] += s.x; ps[1] += s.y; ps[2] += s.z;
        pq[0] += q.x; pq[1] += q.y; pq[2] += q.z;
        accN[e] += k;
    }
}

// What a select leaves in device memory for the host's one read per pass:
// the list's length, ~(the smallest k of a listed pixel) (0: empty list) and
// the samples the pass will add.
struct AccumMeta {
    uint32_t count, nkmin;
    unsigned long long ksum;
};
constexpr uint32_t kSelBlock = 256;
// The select's work-item -> pixel.  Whole frame (BAND false): item b of npix
// is pixel e = b.  Band form (BAND true): the grid covers the band's B.npix
// pixels only, item b is band pixel b -> e = band_pixel(B, b) (pt_path.h);
// e ascends with b, so blocks, bcount and the list keep their order.
template <bool BAND>
__device__ __forceinline__ uint32_t sel_pixel(uint32_t npix, const BandK& B, bool* in) {
    const uint64_t b = (uint64_t)blockIdx.x * kSelBlock + threadIdx.x;
    *in = b < (uint64_t)(BAND ? B.npix : npix);
    return BAND ? (*in ? band_pixel(B, (uint32_t)b) : 0u) : (uint32_t)b;
}
// 1. err of every pixel, the active pixels of each block counted
template <bool BAND>
__global__ __launch_bounds__(kSelBlock) void k_accum_select_count(
    const double* __restrict__ accS, const double* __restrict__ accQ, const uint32_t* __restrict__ accN,
    uint32_t npix, BandK B, AdaptK A, double* __restrict__ err, uint32_t* __restrict__ bcount,
    AccumMeta* __restrict__ meta) {
    __shared__ uint32_t wc[kSelBlock / 64];
    bool in;
    const uint32_t e = sel_pixel<BAND>(npix, B, &in);
    bool act = false;
    uint32_t k = 0;
    if (in) {
        const uint32_t n = accN[e];
        const double er = moment_err(accS + (size_t)e * 3, accQ + (size_t)e * 3, n, A.floor);
        err[e] = er;
        act = adapt_active(n, er, A);
        k = act ? adapt_k(n, A) : 0u;
    }
    const unsigned long long b = __ballot(act);
    uint32_t ks = k, nk = act ? ~k : 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        ks += __shfl_xor(ks, m);
        nk = max(nk, (uint32_t)__shfl_xor(nk, m));
    }
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (lane == 0) {
        wc[w] = (uint32_t)__popcll(b);
        if (b) {
            atomicAdd(&meta->ksum, (unsigned long long)ks);
            atomicMax(&meta->nkmin, nk);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t i = 0; i < kSelBlock / 64; ++i) t += wc[i];
        bcount[blockIdx.x] = t;
    }
}
// 2. one block of 1024: the block counts become their exclusive prefix sums,
// the total is the list's length
__global__ __launch_bounds__(1024) void k_accum_select_scan(uint32_t* __restrict__ bcount, uint32_t nb,
                                                            AccumMeta* __restrict__ meta) {
    __shared__ uint32_t wsum[16];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += 1024u) {   // (block-uniform trip count)
        const uint32_t i = base + t;
        const uint32_t v = i < nb ? bcount[i] : 0u;
        const uint32_t incl = wave_incl_scan(v);
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        uint32_t x = carry + incl - v, total = 0;
        for (uint32_t j = 0; j < 16; ++j) {
            if (j < w) x += wsum[j];
            total += wsum[j];
        }
        if (i < nb) bcount[i] = x;
        carry += total;
        __syncthreads();
    }
    if (t == 0) meta->count = carry;
}
// 3. the active pixels of each block, in order, from the block's offset on
template <bool BAND>
__global__ __launch_bounds__(kSelBlock) void k_accum_select_scatter(
    const double* __restrict__ err, const uint32_t* __restrict__ accN, uint32_t npix, BandK B, AdaptK A,
    const uint32_t* __restrict__ boff, uint32_t* __restrict__ list) {
    __shared__ uint32_t wc[kSelBlock / 64];
    bool in;
    const uint32_t e = sel_pixel<BAND>(npix, B, &in);
    const bool act = in && adapt_active(accN[e], err[e], A);
    const unsigned long long b = __ballot(act);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (lane == 0) wc[w] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t off = boff[blockIdx.x] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    for (uint32_t i = 0; i < w; ++i) off += wc[i];
    if (act) list[off] = e;   // off < the list's length <= npix
}
__global__ __launch_bounds__(256) void k_accum_reset(double* __restrict__ err, uint32_t npix) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e < (uint64_t)npix) err[e] = (double)INFINITY;
}
// Band tiles (include/pt_capi.h): the band's P = B.npix pixels top-first as
// S [P][3], Q [P][3], err [P] f64 and n [P] u32.  A band row is contiguous in
// the accumulator as in the tile (3W f64 of S and of Q, W of err and of n), so
// one work-item moves element u < 3P of S and of Q, and the first P of them
// also pixel u's err and n: every access is an 8- or 4-byte vector access that
// is coalesced along the row.  HBM-bound, one read and one write of the band.
__device__ __forceinline__ bool tile_item(const BandK& B, uint64_t* u, size_t* at3, uint32_t* e) {
    *u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t P = B.npix;
    if (*u >= 3u * P) return false;
    const uint64_t row3 = 3u * (uint64_t)B.W;
    const uint64_t j = *u / row3, c = *u - j * row3;
    *at3 = (size_t)(((uint64_t)(B.H - 1 - B.iy_top) + j * (uint64_t)B.step) * row3 + c);
    *e = *u < P ? band_pixel(B, (uint32_t)*u) : 0u;
    return true;
}
__global__ __launch_bounds__(256) void k_accum_export_band(
    const double* __restrict__ accS, const double* __restrict__ accQ, const double* __restrict__ err,
    const uint32_t* __restrict__ accN, BandK B, double* __restrict__ tS, double* __restrict__ tQ,
    double* __restrict__ tE, uint32_t* __restrict__ tN) {
    uint64_t u;
    size_t at3;
    uint32_t e;
    if (!tile_item(B, &u, &at3, &e)) return;
    tS[u] = accS[at3];
    tQ[u] = accQ[at3];
    if (u < (uint64_t)B.npix) {
        tE[u] = err[e];
        tN[u] = accN[e];
    }
}
__global__ __launch_bounds__(256) void k_accum_import_band(
    const double* __restrict__ tS, const double* __restrict__ tQ, const double* __restrict__ tE,
    const uint32_t* __restrict__ tN, BandK B, double* __restrict__ accS, double* __restrict__ accQ,
    double* __restrict__ err, uint32_t* __restrict__ accN) {
    uint64_t u;
    size_t at3;
    uint32_t e;
    if (!tile_item(B, &u, &at3, &e)) return;
    accS[at3] = tS[u];
    accQ[at3] = tQ[u];
    if (u < (uint64_t)B.npix) {
        err[e] = tE[u];
        accN[e] = tN[u];
    }
}
// S / n (0 where n = 0) as a framebuffer of k_render's layout (the whole frame)
__global__ __launch_bounds__(256) void k_accum_resolve(const double* __restrict__ accS,
                                                       const uint32_t* __restrict__ accN, uint32_t npix,
                                                       int32_t out_f64, void* __restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint64_t)npix) return;
    const uint32_t n = accN[e];
    const double dn = (double)n;
    const double* s = accS + e * 3;
    const double r = n ? s[0] / dn : 0.0, g = n ? s[1] / dn : 0.0, b = n ? s[2] / dn : 0.0;
    if (out_f64) {
        double* o = (double*)out + e * 3;
        o[0] = r; o[1] = g; o[2] = b;
    } else {
        float* o = (float*)out + e * 3;
        o[0] = (float)r; o[1] = (float)g; o[2] = (float)b;
    }
}

// the origins the filter's bounds cover: within the surface frame's box
// (xs), within the box with the eye (xa); outside both -> forced f64
__device__ __forceinline__ bool in_box(F3 o, float x) {
    return fabsf(o.x) <= x && fabsf(o.y) <= x && fabsf(o.z) <= x;
}

// pt_signal: one 64-bit flag store after the stream's earlier work, released
// at system scope (a vector store; the host or a peer polls the flag)
__global__ __launch_bounds__(64) void k_signal(uint64_t* flag, uint64_t v) {
    if (threadIdx.x == 0) __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(256) void k_intersect(SceneK S, const double* __restrict__ rays,
                                                   int64_t n, float xs, float xa,
                                                   int32_t* __restrict__ out_tri,
                                                   double* __restrict__ out_p) {
    __shared__ double spill[kSpillSlots][256];
    const Spill sp{&spill[0][threadIdx.x], 256};
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const D3 o = ld3(rays + 6 * i), d = ld3(rays + 6 * i + 3);
    const bool in_s = in_box(to_f3(o - ld3(S.center_s)), xs);
    const bool in_a = in_box(to_f3(o - ld3(S.center)), xa);
    D3 P = d3(0, 0, 0);
    Counters c;
    // the uniform units take either frame (eye = !in_s), but the BVH walk
    // always runs in the frame with the eye (its boxes' inflation assumes
    // |o - center| <= xa): scenes with a BVH need in_a for the filter
    const bool fast = S.n_bnode > 0 ? in_a : (in_s || in_a);
    const int t = fast ? closest<false, false>(S, o, d, -1, sp, &P, &c, !in_s)
                       : closest<true, false>(S, o, d, -1, sp, &P, &c, true);
    out_tri[i] = t;
    out_p[3 * i] = P.x; out_p[3 * i + 1] = P.y; out_p[3 * i + 2] = P.z;
}

__global__ __launch_bounds__(256) void k_color(SceneK S, const int32_t* __restrict__ obj,
                                               const double* __restrict__ point,
                                               const double* __restrict__ normal,
                                               const double* __restrict__ u, int64_t n, float xs,
                                               float xa, double* __restrict__ out) {
    __shared__ double spill[kSpillSlots][256];
    const Spill sp{&spill[0][threadIdx.x], 256};
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const D3 P = ld3(point + 3 * i);
    double uu[12];
    for (int j = 0; j < 12; ++j) uu[j] = u[12 * i + j];
    // nee() tests the uniform units in the surface frame and the BVH in the
    // frame with the eye: the filter needs the point inside both boxes
    const bool ok = in_box(to_f3(P - ld3(S.center_s)), xs) && in_box(to_f3(P - ld3(S.center)), xa);
    Counters c;
    const D3 col = ok ? nee<false, false>(S, P, ld3(normal + 3 * i), obj[i], -1, uu, sp, &c)
                          : nee<true, false>(S, P, ld3(normal + 3 * i), obj[i], -1, uu, sp, &c);
    out[3 * i] = col.x; out[3 * i + 1] = col.y; out[3 * i + 2] = col.z;
}

// ------------------------------- wavefront, list form (pt_accum) --
// The list form of the wavefront render (BVH scenes, render_wavefront from
// pt_accum_render_stats): k_wf_shade_list (pt_shade.h) for k_wf_shade, and the two kernels
// below for k_wf_primary and k_wf_final; the walk kernels and the sort only
// see the path slots, the query records and the lists.
// The primary rays, one work-item per list entry (the entry's `split` slots
// share it): CQP[entry], spill home in the entry's first slot, list entry =
// entry (k_wf_closest's wshift = split_log2).
__global__ __launch_bounds__(256) void k_wf_primary_list(SceneK S, ListK R, const uint32_t* __restrict__ list,
                                                         const uint32_t* __restrict__ accN,
                                                         WfPath* __restrict__ W, WfClosestQ* __restrict__ CQP,
                                                         int32_t* __restrict__ qlist, int32_t* counters) {
    const uint32_t entry = blockIdx.x * 256u + threadIdx.x;
    const uint32_t want = wf_primary_step(S, WfActive{R, list, accN}, entry, W, CQP);
    wf_append((want & kWfWantClosest) != 0, counters, qlist, (int32_t)entry);
}
// k_render_list's epilogue over the slots' sums (home[6][slots], one block of
// 256 per 256 slots): an entry's slots reduce S and Q in store_pixel's xor
// order and slot 0 adds them to the accumulator with plain loads and stores.
__global__ __launch_bounds__(256) void k_wf_final_list(ListK R, const uint32_t* __restrict__ list,
                                                       const double* __restrict__ home, uint32_t slots,
                                                       double* __restrict__ accS, double* __restrict__ accQ,
                                                       uint32_t* __restrict__ accN) {
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;   // < slots
    const uint32_t entry = tid >> R.split_log2, c = tid & (R.split - 1u);
    const uint32_t e = entry < R.n_list ? list[entry] : 0xffffffffu;
    const bool valid = e < R.npix;   // the same for all slots of an entry
    const double* h = home + tid;
    D3 s = d3(0, 0, 0), q = d3(0, 0, 0);
    if (valid) {
        s = d3(h[0], h[slots], h[2 * (size_t)slots]);
        q = d3(h[3 * (size_t)slots], h[4 * (size_t)slots], h[5 * (size_t)slots]);
    }
    for (uint32_t m = 1; m < R.split; m <<= 1) {
        s.x += __shfl_xor(s.x, (int)m); s.y += __shfl_xor(s.y, (int)m); s.z += __shfl_xor(s.z, (int)m);
        q.x += __shfl_xor(q.x, (int)m); q.y += __shfl_xor(q.y, (int)m); q.z += __shfl_xor(q.z, (int)m);
    }
    if (valid && c == 0) {
        const uint32_t k = adapt_k(accN[e], R.A);
        if (k > 0) {
            double* ps = accS + (size_t)e * 3;
            double* pq = accQ + (size_t)e * 3;
            ps[0] += s.x; ps[1] += s.y; ps[2] += s.z;
            pq[0] += q.x; pq[1] += q.y; pq[2] += q.z;
            accN[e] += k;
        }
    }
}

// Sections of a scratch buffer, handed out front to back (base null: only the
// sizes, `at` the bytes needed so far)
struct Bump {
    char* base;
    size_t at = 0;
    template <class T>
    T* take(size_t n, size_t align = 256) {
        at = (at + align - 1) / align * align;
        T* p = base ? (T*)(base + at) : nullptr;
        at += n * sizeof(T);
        return p;
    }
};

// ---------------------------------------------------------------- API --
struct pt_scene {
    int device = 0;
    uint64_t fingerprint = 0;   // of the scene descriptor (pt_render_multi: one scene on every handle)
    bool has_lens = false;      // created by pt_scene_create_lens with a lens (PT_FLAG_LENS is allowed)
    pt_launch_info last{};      // the last launch on this handle (pt_last_launch_info; host side only)
    int n_cu = 256;   // compute units of the device (MI355X: 256 in 8 XCDs)
    HostScene host;
    SceneK dev{};
    float xb_surf = 0.f, xb_all = 0.f;   // origin boxes of the two filter frames
    void* blob = nullptr;          // all scene tables, one allocation
    StatsDev* stats = nullptr;
    void* out_dev = nullptr;       // pt_render's staging buffer
    size_t out_cap = 0;
    hipStream_t stream = nullptr;  // pt_render's own stream
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    // wavefront path (BVH scenes): path records, query records, query lists
    // and counters, one allocation grown on demand
    void* wf = nullptr;
    size_t wf_bytes = 0;
    hipStream_t wf_side = nullptr;             // the closest walks run beside the shadow walks
    hipEvent_t wf_ev_shade = nullptr, wf_ev_walk = nullptr;
    std::vector<hipEvent_t> prof_ev;           // PT_FLAG_KERNEL_TIMES
};

namespace {
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// Origins handed to the filter must lie in the box its bounds assume: the
// largest centred coordinate of the triangles (surface frame), or of the
// triangles and the eye (frame with the eye), as prepare_scene's X.
float box_bound(const HostScene& H, bool with_eye) {
    double X = 0.0;
    const SceneK& K = H.k;
    const double* c = with_eye ? K.center : K.center_s;
    for (const TriD& T : H.trid) {
        const double* vs[3] = {T.v1, T.v2, T.v3};
        for (int v = 0; v < 3; ++v)
            for (int i = 0; i < 3; ++i) X = std::max(X, fabs(vs[v][i] - c[i]));
    }
    if (with_eye)
        for (int i = 0; i < 3; ++i) X = std::max(X, fabs(K.eye[i] - c[i]));
    return (float)X;
}
}  // namespace

template <typename T>
static int dev_alloc_copy(T** d, const T* h, size_t n) {
    HIPCHK(hipMalloc((void**)d, n * sizeof(T) + 16));
    if (h) HIPCHK(hipMemcpy(*d, h, n * sizeof(T), hipMemcpyHostToDevice));
    return PT_OK;
}

#if defined(PT_PHASE_CLOCKS)
// dev builds only (scripts/phase_clocks.py): the phase clocks of pt_path.h
extern "C" int pt_debug_phase_clocks(unsigned long long* out, int reset) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(pt_phase_clk), 8 * sizeof(unsigned long long)));
    if (reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(pt_phase_clk), z, sizeof(z)));
    }
    return PT_OK;
}
#endif

extern "C" {

int pt_api_version(void) { return PT_API_VERSION; }

// The content hash of the sources this library was compiled from
// (pathtracerpython_amd/build.py passes it as PT_BUILD_ID; the marker lets the
// build read it back from the file without loading it).
#ifndef PT_BUILD_ID
#error "PT_BUILD_ID (the sources' content hash) must be defined: build with pathtracerpython_amd/build.py"
#endif
static const char pt_build_id_str[] = "PT_BUILD_ID=" PT_BUILD_ID;
const char* pt_build_id(void) { return pt_build_id_str + 12; }

// test hook (tests/test_gpu.py): pt_render_multi fails while dealing band i
static std::atomic<int32_t> g_fault_multi{-1};
int pt_test_fault_inject(int32_t multi_band) {
    g_fault_multi.store(multi_band);
    return PT_OK;
}

const char* pt_last_error(void) { return g_err.c_str(); }

int pt_device_count(int32_t* count) {
    if (!count) return fail(PT_EINVAL, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count = n;
    return PT_OK;
}

void pt_scene_destroy(pt_scene* s) {
    if (!s) return;
    {
        DeviceGuard g(s->device);
        if (s->blob) (void)hipFree(s->blob);
        if (s->stats) (void)hipFree(s->stats);
        if (s->out_dev) (void)hipFree(s->out_dev);
        if (s->wf) (void)hipFree(s->wf);
        if (s->wf_ev_shade) (void)hipEventDestroy(s->wf_ev_shade);
        if (s->wf_ev_walk) (void)hipEventDestroy(s->wf_ev_walk);
        if (s->wf_side) (void)hipStreamDestroy(s->wf_side);
        for (hipEvent_t e : s->prof_ev) (void)hipEventDestroy(e);
        if (s->ev0) (void)hipEventDestroy(s->ev0);
        if (s->ev1) (void)hipEventDestroy(s->ev1);
        if (s->stream) (void)hipStreamDestroy(s->stream);
    }
    delete s;
}

int pt_scene_create_on(const pt_scene_desc* desc, int32_t device, pt_scene** out) {
    if (!out) return fail(PT_EINVAL, "null output handle");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PT_ENODEV, "no HIP device visible (the MI355X path needs a gfx950 GPU)");
    if (device < 0 || device >= ndev)
        return fail(PT_EINVAL, "device " + std::to_string(device) + " out of range (" +
                                   std::to_string(ndev) + " visible)");
    DeviceGuard g(device);
    return pt_scene_create(desc, out);
}

static int scene_create(const pt_scene_desc* desc, const pt_lens* lens, pt_scene** out,
                        const double* ray_box = nullptr);
int pt_scene_create_lens(const pt_scene_desc* desc, int32_t device, const pt_lens* lens, pt_scene** out) {
    if (!lens) return pt_scene_create_on(desc, device, out);
    if (!out) return fail(PT_EINVAL, "null output handle");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PT_ENODEV, "no HIP device visible (the MI355X path needs a gfx950 GPU)");
    if (device == -1) return scene_create(desc, lens, out);   // the current device
    if (device < 0 || device >= ndev)
        return fail(PT_EINVAL, "device " + std::to_string(device) + " out of range (" +
                                   std::to_string(ndev) + " visible)");
    DeviceGuard g(device);
    return scene_create(desc, lens, out);
}

int pt_scene_create_rays(const pt_scene_desc* desc, int32_t device, const double box[6], pt_scene** out) {
    if (!box) return pt_scene_create_on(desc, device, out);
    if (!out) return fail(PT_EINVAL, "null output handle");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PT_ENODEV, "no HIP device visible (the MI355X path needs a gfx950 GPU)");
    if (device == -1) return scene_create(desc, nullptr, out, box);   // the current device
    if (device < 0 || device >= ndev)
        return fail(PT_EINVAL, "device " + std::to_string(device) + " out of range (" +
                                   std::to_string(ndev) + " visible)");
    DeviceGuard g(device);
    return scene_create(desc, nullptr, out, box);
}

// FNV-1a over the descriptor's arrays and constants
static void fnv(uint64_t* h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) *h = (*h ^ b[i]) * 0x100000001b3ull;
}
static uint64_t scene_fingerprint(const pt_scene_desc* d) {
    uint64_t h = 0xcbf29ce484222325ull;
    const size_t T = (size_t)d->n_tri;
    fnv(&h, &d->n_tri, 3 * sizeof(int32_t));
    fnv(&h, d->tri_v, 9 * T * sizeof(double));
    fnv(&h, d->tri_n, 3 * T * sizeof(double));
    fnv(&h, d->tri_area, T * sizeof(double));
    fnv(&h, d->tri_obj, T * sizeof(int32_t));
    fnv(&h, d->mat, 8 * (size_t)d->n_obj * sizeof(double));
    fnv(&h, d->eye, sizeof(d->eye) + sizeof(d->ortho) + sizeof(d->ambient) + sizeof(d->light_rgb));
    return h;
}

int pt_scene_create(const pt_scene_desc* desc, pt_scene** out) { return scene_create(desc, nullptr, out); }

static int scene_create(const pt_scene_desc* desc, const pt_lens* lens, pt_scene** out, const double* ray_box) {
    if (!out) return fail(PT_EINVAL, "null output handle");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PT_ENODEV, "no HIP device visible (the MI355X path needs a gfx950 GPU)");
    pt_scene* s = new pt_scene();
    std::string err = prepare_scene(desc, &s->host, lens, ray_box);
    if (!err.empty()) { delete s; return fail(PT_EINVAL, err); }
    s->has_lens = lens != nullptr;
    if (hipGetDevice(&s->device) != hipSuccess) { delete s; return fail(PT_EHIP, "hipGetDevice failed"); }
    s->fingerprint = scene_fingerprint(desc);   // (prepare_scene checked the arrays)
    if (lens) fnv(&s->fingerprint, lens, sizeof(*lens));   // (another frame: no mixing with lens-free handles)
    if (ray_box) fnv(&s->fingerprint, ray_box, 6 * sizeof(double));   // (likewise)
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, s->device) == hipSuccess) {
        if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
            std::string arch = prop.gcnArchName;
            delete s;
            return fail(PT_ENODEV, "device is " + arch + ", this build targets gfx950 only");
        }
        if (prop.multiProcessorCount > 0) s->n_cu = prop.multiProcessorCount;
    }
    HostScene& H = s->host;
    constexpr int kArrays = 15;
    const size_t sz[kArrays] = {H.unit.size() * sizeof(UnitF), H.trid.size() * sizeof(TriD),
                                H.tris.size() * sizeof(TriS), H.tri_obj.size() * sizeof(int32_t),
                                H.mat.size() * sizeof(Mat), H.light_tri.size() * sizeof(int32_t),
                                H.light_cum.size() * sizeof(double),
                                H.tri_grp.size() * sizeof(int32_t),
                                H.bnode.size() * sizeof(BNode), H.bunit.size() * sizeof(UnitF),
                                H.cnode.size() * sizeof(CNode), H.qnode.size() * sizeof(QNode),
                                H.bunitc.size() * sizeof(UnitC), H.unit_eye.size() * sizeof(UnitF),
                                H.kd.size() * sizeof(double)};
    const void* src[kArrays] = {H.unit.data(), H.trid.data(), H.tris.data(), H.tri_obj.data(),
                                H.mat.data(), H.light_tri.data(), H.light_cum.data(),
                                H.tri_grp.data(), H.bnode.data(), H.bunit.data(), H.cnode.data(),
                                H.qnode.data(), H.bunitc.data(), H.unit_eye.data(), H.kd.data()};
    size_t off[kArrays], total = 0;
    for (int i = 0; i < kArrays; ++i) { off[i] = total; total += align_up(sz[i]); }
    int rc = PT_OK;
    auto cleanup = [&](int code, const std::string& m) { pt_scene_destroy(s); return fail(code, m); };
    if (hipMalloc(&s->blob, total) != hipSuccess) return cleanup(PT_ENOMEM, "hipMalloc scene tables");
    for (int i = 0; i < kArrays; ++i)
        if (sz[i] && hipMemcpy((char*)s->blob + off[i], src[i], sz[i], hipMemcpyHostToDevice) != hipSuccess)
            return cleanup(PT_EHIP, "hipMemcpy scene tables");
    if (hipMalloc((void**)&s->stats, sizeof(StatsDev)) != hipSuccess) return cleanup(PT_ENOMEM, "hipMalloc stats");
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess)
        return cleanup(PT_EHIP, "stream/event creation");
    s->dev = H.k;
    char* b = (char*)s->blob;
    s->dev.unit = (const UnitF*)(b + off[0]);
    s->dev.trid = (const TriD*)(b + off[1]);
    s->dev.tris = (const TriS*)(b + off[2]);
    s->dev.tri_obj = (const int32_t*)(b + off[3]);
    s->dev.mat = (const Mat*)(b + off[4]);
    s->dev.light_tri = (const int32_t*)(b + off[5]);
    s->dev.light_cum = (const double*)(b + off[6]);
    s->dev.tri_grp = (const int32_t*)(b + off[7]);
    s->dev.bnode = (const BNode*)(b + off[8]);
    s->dev.bunit = (const UnitF*)(b + off[9]);
    s->dev.cnode = (const CNode*)(b + off[10]);
    s->dev.qnode = (const QNode*)(b + off[11]);
    s->dev.bunitc = H.bunitc.empty() ? nullptr : (const UnitC*)(b + off[12]);
    s->dev.unit_eye = (const UnitF*)(b + off[13]);
    s->dev.kd = (const double*)(b + off[14]);
    s->xb_surf = box_bound(H, false);
    s->xb_all = box_bound(H, true);
    *out = s;
    return rc;
}

int pt_band_rows(const pt_render_params* p, int32_t* rows) {
    if (!p || !rows) return fail(PT_EINVAL, "null argument");
    int32_t first;
    if (!band_layout(p, &first, rows)) return fail(PT_EINVAL, "bad row_step/row_phase");
    return PT_OK;
}

// The launch rules — the argument checks, the lanes per pixel (choose_split),
// the launch records, the work-items and the route — are pt_plan.h's; here
// they meet the handles.  PLANCHK: a check's message is a PT_EINVAL.
#define PLANCHK(expr) do { const std::string m_ = (expr); if (!m_.empty()) return fail(PT_EINVAL, m_); } while (0)
static PlanScene plan_scene(const pt_scene* s) {
    return PlanScene{s->dev.n_bnode > 0, s->dev.n_qnode > 0 && s->dev.qstack <= kWalkStack, s->n_cu, s->has_lens,
                     s->host.frame_x};
}
// Launches on one handle share its scratch (wavefront state, counters,
// events): every launch is ordered after the previous one, whatever stream
// that one ran on, and bracketed by ev0 / ev1 (pt_last_kernel_ms).
static int launch_begin(pt_scene* s, hipStream_t st) {
    if (s->timed) HIPCHK(hipStreamWaitEvent(st, s->ev1, 0));
    HIPCHK(hipEventRecord(s->ev0, st));
    return PT_OK;
}
static int launch_end(pt_scene* s, hipStream_t st) {
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev1, st));
    s->timed = true;
    return PT_OK;
}

// Walk kernels: node-phase exit threshold (lanes still descending) and
// persistent grid size.  At 16M slots (K5 512^2 x 64 spp) the threshold
// 4 / 8 / 12 / 16 / 20 / 24 / 32 / 48 -> 149 / 140 / 134 / 131 / 129 / 128 /
// 130 / 174 ms; grids of 1 / 2 / 3 / 4 / 16 blocks per CU -> 271 / 174 / 169
// / 178 / 188 ms.  Compile-time (-D) so tuning builds can sweep them; the
// shipped library has no run-time knobs.
// Round 2 re-sweep (512^2 x 64 spp render, both walks): 16 / 24 / 32 / 40 /
// 48 -> 114.3 / 110.5 / 108.0 / 107.8 / 109.5 ms; the one-ray shadow walk's
// threshold 16 / 24 / 32 / 40 / 48 -> 100.7 / 98.8 / 97.4 / 96.9 / 96.9 ms.
// At the K5 bench size with 64M slots (1024^2 x 256 spp, ms): shadow / closest
// 40/32 1372-1382, 32/32 1407, 48/32 1366, 40/40 1370, 48/40 1349, 48/48
// 1351, 56/48 1359, 64/56 1885 (64: the node phase never ends early).
#ifndef PT_WF_THR_SHADOW
#define PT_WF_THR_SHADOW 48
#endif
#ifndef PT_WF_THR_CLOSEST
#define PT_WF_THR_CLOSEST 40
#endif
#ifndef PT_WF_SHADOW_BLOCKS_PER_CU
#define PT_WF_SHADOW_BLOCKS_PER_CU 5
#endif
#ifndef PT_WF_CLOSEST_BLOCKS_PER_CU
#define PT_WF_CLOSEST_BLOCKS_PER_CU 5
#endif
#ifndef PT_WF_CONCURRENT   // the two walks of a step on two streams
#define PT_WF_CONCURRENT 1
#endif

// The wavefront render of a BVH scene (pt_wavefront.h): per step one shade
// launch over the path slots, then the two persistent walk launches over the
// queries it appended.  A slot runs at most n_samples x bounces bounces plus
// the primary ray, so that many steps (+1 to finish the last bounce) drain
// every slot; steps after that would find no work.
// The walk launches: the <UC, COUNT> instantiation for a scene whose BVH units
// have the 64-B form (SceneK::bunitc) and for a PT_FLAG_WALK_COUNT launch.
static void launch_wf_closest(bool uc, bool count, unsigned blocks, hipStream_t on, const SceneK& S, WfPath* W,
                              WfClosestQ* Q, const int32_t* list, int32_t* counters, unsigned long long* wc,
                              int* ovf_ref, uint16_t* ovf_dist, uint32_t wshift) {
    const auto k = uc ? (count ? k_wf_closest<true, true> : k_wf_closest<true, false>)
                      : (count ? k_wf_closest<false, true> : k_wf_closest<false, false>);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, on, S, W, Q, list, counters, PT_WF_THR_CLOSEST, wc, ovf_ref,
                       ovf_dist, wshift);
}
static void launch_wf_shadow(bool uc, bool count, unsigned blocks, hipStream_t on, const SceneK& S, WfPath* W,
                             WfShadowQ* SQ, const int32_t* list, int32_t* counters, unsigned long long* wc,
                             int* ovf) {
    const auto k = uc ? (count ? k_wf_shadow<true, true> : k_wf_shadow<true, false>)
                      : (count ? k_wf_shadow<false, true> : k_wf_shadow<false, false>);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, on, S, W, SQ, list, counters, PT_WF_THR_SHADOW, wc, ovf);
}
}  // extern "C"

// What the loop reads of a pass.  Its three launches (the shade step, step 0's
// primary queries where the slots do not start their own, the final reduction)
// come from the caller, who knows the form (pt_render_device, pt_radiance_device,
// pt_accum_render_stats); each is called with the launch's buffers (B below).
struct WfPass {
    uint32_t n_prim;       // primary queries (one per pixel / list entry / record)
    uint32_t split_log2;   // slots per query
    int32_t max_k;         // the most samples the pass adds to a query
    int32_t bounces;
    bool own;              // a primary query per sample, in the slots' own records: no primary launch
    bool moments;          // the slots' moment home [6][slots]
};
template <class Shade, class Primary, class Finish>
static int render_wavefront(pt_scene* s, const WfPass& P, dim3 grid, hipStream_t st, uint32_t flags, pt_stats* stats,
                            const Shade& shade, const Primary& primary, const Finish& finish) {
    const size_t slots = (size_t)grid.x * 256;
    const uint32_t n_prim = P.n_prim, split_log2 = P.split_log2;
    const int32_t split = (int32_t)(1u << split_log2);
    const int32_t per_slot = (P.max_k + split - 1) / split;   // samples per slot
    const bool own = P.own, moments = P.moments;
    const int32_t steps = per_slot * (P.bounces + (own ? 1 : 0)) + 2;
    const unsigned sh_blocks =
        std::max(1u, std::min<unsigned>(grid.x, (unsigned)PT_WF_SHADOW_BLOCKS_PER_CU * (unsigned)s->n_cu));
    const unsigned cl_blocks =
        std::max(1u, std::min<unsigned>(grid.x, (unsigned)PT_WF_CLOSEST_BLOCKS_PER_CU * (unsigned)s->n_cu));
    // the launch's buffers in s->wf, each section on a 256-B boundary
    struct {
        WfPath* W;
        WfShadowQ* SQ;
        WfClosestQ* CQ;
        int32_t *lists, *counters;   // [4 slots], [4] (the shade kernels' queue counters)
        int* ovf_s;                  // walk-stack overflow (entries below the shared-memory part):
        int* ovf_cr;                 // 4 B per entry and shadow lane, 4 + 2 B per entry and closest lane
        uint16_t* ovf_cd;
        WfClosestQ* CQP;             // the primary queries
        uint16_t* keys;              // the shadow list's sort keys [3 slots]
        int32_t* lists_o;            // the sorted shadow list [3 slots]
        uint32_t *bin_hist, *bin_rowsum, *bin_base;   // the sort's count matrix (its rows' prefix sums in
                                                      // place), the row totals and their scan
        double* home;                // the moment home [6][slots] (the list form; rays with S, Q)
        uint32_t slots;              // (for the pass's launches)
        int32_t* closest_list;       // the closest list: lists + 3 slots
    } B;
    auto carve = [&](char* base) -> size_t {   // returns the bytes carved
        Bump m{base};
        const size_t ovf_n = (size_t)kWalkStackGlobal;
        B.W = m.take<WfPath>(slots);
        B.SQ = m.take<WfShadowQ>(slots);
        B.CQ = m.take<WfClosestQ>(slots);
        B.lists = m.take<int32_t>(4 * slots);
        B.counters = m.take<int32_t>(64);
        B.ovf_s = m.take<int>(ovf_n * sh_blocks * 256);
        B.ovf_cr = m.take<int>(ovf_n * cl_blocks * 256);
        B.ovf_cd = m.take<uint16_t>(ovf_n * cl_blocks * 256);
        B.CQP = m.take<WfClosestQ>(n_prim);
        B.keys = m.take<uint16_t>(3 * slots);
        B.lists_o = m.take<int32_t>(3 * slots);
        B.bin_hist = m.take<uint32_t>((size_t)kBins * kBinBlocks);
        B.bin_rowsum = m.take<uint32_t>(kBins);
        B.bin_base = m.take<uint32_t>(kBins);
        B.home = m.take<double>(moments ? 6 * slots : 0);
        return m.at;
    };
    const size_t need = carve(nullptr) + 256;
    if (need > s->wf_bytes) {
        if (s->wf) (void)hipFree(s->wf);
        s->wf = nullptr;
        s->wf_bytes = 0;
        if (hipMalloc(&s->wf, need) != hipSuccess) return fail(PT_ENOMEM, "hipMalloc wavefront buffers");
        s->wf_bytes = need;
    }
    if (!s->wf_side) {
        HIPCHK(hipStreamCreateWithFlags(&s->wf_side, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&s->wf_ev_shade, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&s->wf_ev_walk, hipEventDisableTiming));
    }
    carve((char*)s->wf);
    int32_t* const closest_list = B.closest_list = B.lists + 3 * slots;
    B.slots = (uint32_t)slots;
    bool sorted = false;   // this step's shadow list is in lists_o
    auto bin_sort = [&]() -> hipError_t {   // (the device reads the list's length: no host wait)
        hipLaunchKernelGGL(k_bin_hist, dim3(kBinBlocks), dim3(256), 0, st, (const uint16_t*)B.keys,
                           (const int32_t*)B.counters, B.bin_hist);
        hipLaunchKernelGGL(k_bin_rows, dim3(kBins / 4), dim3(256), 0, st, B.bin_hist, (const int32_t*)B.counters,
                           B.bin_rowsum);
        hipLaunchKernelGGL(k_bin_base, dim3(1), dim3(1024), 0, st, (const uint32_t*)B.bin_rowsum, B.bin_base);
        hipLaunchKernelGGL(k_bin_scatter, dim3(kBinBlocks), dim3(256), 0, st, (const uint16_t*)B.keys,
                           (const int32_t*)B.lists, (const int32_t*)B.counters, (const uint32_t*)B.bin_hist,
                           (const uint32_t*)B.bin_base, B.lists_o);
        sorted = true;
        return hipGetLastError();
    };
    const bool wcount = (flags & PT_FLAG_WALK_COUNT) != 0 && stats;
    const bool times = (flags & PT_FLAG_KERNEL_TIMES) != 0 && stats;
    unsigned long long* wc = (unsigned long long*)s->stats;   // [0..2] shadow, [3..5] closest
    // per-kernel HIP events (PT_FLAG_KERNEL_TIMES): shade, shadow, closest, the
    // shadow list's sort x (start, end) per step
    constexpr int kEv = 8;
    if (times) {
        const size_t ne = (size_t)steps * kEv;
        while (s->prof_ev.size() < ne) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            s->prof_ev.push_back(e);
        }
    }
    auto mark = [&](int32_t step, int k, int end, hipStream_t on) -> hipError_t {
        return times ? hipEventRecord(s->prof_ev[(size_t)step * kEv + k * 2 + end], on) : hipSuccess;
    };
    RCCHK(launch_begin(s, st));
    if (wcount) HIPCHK(hipMemsetAsync(s->stats, 0, sizeof(StatsDev), st));
    s->last = pt_launch_info{PT_PATH_WAVEFRONT, steps, split, flags};
    for (int32_t step = 0; step < steps; ++step) {
        HIPCHK(hipMemsetAsync(B.counters, 0, 4 * sizeof(int32_t), st));
        HIPCHK(mark(step, 0, 0, st));
        const dim3 sgrid((unsigned)((slots + kShadeBlock - 1) / kShadeBlock)), pgrid((n_prim + 255) / 256);
        shade(B, step, sgrid);
        if (step == 0 && !own) primary(B, pgrid);
        HIPCHK(mark(step, 0, 1, st));
        sorted = false;
        if (step + 1 < steps) {
            // the two walks only read the shade step's output and write
            // disjoint records: the closest walks run on a side stream
            // (PT_FLAG_KERNEL_TIMES launches run them one after the other on
            // one stream, so each walk's HIP-event time is its own time on
            // the whole chip, not the stretches it waits for the other's CUs)
            const bool side = PT_WF_CONCURRENT && !times;
            hipStream_t cs = side ? s->wf_side : st;
            if (side) {
                HIPCHK(hipEventRecord(s->wf_ev_shade, st));
                HIPCHK(hipStreamWaitEvent(s->wf_side, s->wf_ev_shade, 0));
            }
            HIPCHK(mark(step, 2, 0, cs));
            // step 0 walks the primary queries (CQP, one per pixel / entry, the
            // spill home in its first slot), later steps the slots' (CQ)
            const bool prim = step == 0 && !own;
            launch_wf_closest(s->dev.bunitc != nullptr, wcount, cl_blocks, cs, s->dev, B.W, prim ? B.CQP : B.CQ,
                              closest_list, B.counters + 2, wc + 3, B.ovf_cr, B.ovf_cd, prim ? split_log2 : 0u);
            HIPCHK(mark(step, 2, 1, cs));
            if (side) HIPCHK(hipEventRecord(s->wf_ev_walk, s->wf_side));
            // the shadow list sorted by the origin's cell (the device reads
            // its length) while the closest walks, unsorted, already run
            if (step > 0) {   // (step 0: the primary rays)
                HIPCHK(mark(step, 3, 0, st));
                HIPCHK(bin_sort());
                HIPCHK(mark(step, 3, 1, st));
            }
            HIPCHK(mark(step, 1, 0, st));
            launch_wf_shadow(s->dev.bunitc != nullptr, wcount, sh_blocks, st, s->dev, B.W, B.SQ,
                             sorted ? B.lists_o : B.lists, B.counters, wc, B.ovf_s);
            HIPCHK(mark(step, 1, 1, st));
            if (side) HIPCHK(hipStreamWaitEvent(st, s->wf_ev_walk, 0));
        }
    }
    finish(B);
    RCCHK(launch_end(s, st));
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        if (wcount || times) HIPCHK(hipStreamSynchronize(st));
        if (wcount) {
            StatsDev h;
            HIPCHK(hipMemcpy(&h, s->stats, sizeof(h), hipMemcpyDeviceToHost));
            stats->shadow_queries = h.v[0];
            stats->shadow_node_visits = h.v[1];
            stats->shadow_leaf_units = h.v[2];
            stats->closest_queries = h.v[3];
            stats->closest_node_visits = h.v[4];
            stats->closest_leaf_units = h.v[5];
        }
        if (times) {
            double t[4] = {0, 0, 0, 0};
            uint64_t n[4] = {0, 0, 0, 0};
            for (int32_t step = 0; step < steps; ++step)
                for (int k = 0; k < 4; ++k) {
                    if (k > 0 && step + 1 >= steps) continue;
                    if (k == 3 && step == 0) continue;   // (no sort before the primary walks)
                    float ms = 0.f;
                    HIPCHK(hipEventElapsedTime(&ms, s->prof_ev[(size_t)step * kEv + k * 2],
                                               s->prof_ev[(size_t)step * kEv + k * 2 + 1]));
                    t[k] += ms;
                    ++n[k];
                }
            stats->shade_ms = t[0]; stats->shadow_ms = t[1]; stats->closest_ms = t[2];
            stats->shade_launches = n[0]; stats->shadow_launches = n[1]; stats->closest_launches = n[2];
            stats->sort_ms = t[3]; stats->sort_launches = n[3];
        }
    }
    return PT_OK;
}

extern "C" {

int pt_render_device(pt_scene* s, const pt_render_params* p, void* out_dev, void* stream,
                     pt_stats* stats) {
    PLANCHK(validate(p));
    if (!s) return fail(PT_EINVAL, "null scene");
    const PlanScene ps = plan_scene(s);
    PLANCHK(check_scene(p->flags, ps));
    int32_t first = 0, rows = 0;
    band_layout(p, &first, &rows);
    if (rows == 0) return PT_OK;
    if (!out_dev) return fail(PT_EINVAL, "null output");
    DeviceGuard g(s->device);
    hipStream_t st = (hipStream_t)stream;
    RenderK R;
    LaunchPlan L;
    PLANCHK(plan_frame(p, ps, first, rows, &R, &L));
    const bool count = (p->flags & PT_FLAG_COUNT) != 0;
    const bool f64 = (p->flags & PT_FLAG_FORCE_F64) != 0, bvh = ps.bvh;
    const bool aa = (p->flags & PT_FLAG_AA) != 0, lens = (p->flags & PT_FLAG_LENS) != 0;
    if (L.wavefront) {
        // The frame form of render_wavefront.  An antialiased launch has no
        // shared primary query: k_wf_shade_aa starts a query per sample, so a
        // sample takes bounces + 1 steps, step 0's closest walk is over the
        // slots' own records, and CQP stays unused.  A thin-lens launch is of
        // that form with or without PT_FLAG_AA — every sample has its own
        // origin — through the kernels of pt_shade_lens.hip.
        const dim3 grid((unsigned)L.wf_blocks);
        const WfPass P{R.npix, R.split_log2, R.spp, R.bounces, aa || lens, false};
        return render_wavefront(
            s, P, grid, st, p->flags, stats,
            [&](const auto& B, int32_t step, dim3 sgrid) {
                if (lens)   // (a lens point per sample; validate: never with the stats flags)
                    pt_wf_shade_lens(aa, sgrid, st, s->dev, R, step, B.W, B.SQ, B.CQ, B.lists, B.counters, B.slots,
                                     B.keys);
                else if (aa)   // (the slots start their own primary queries)
                    hipLaunchKernelGGL(k_wf_shade_aa, sgrid, dim3(kShadeBlock), 0, st, s->dev, R, step, B.W, B.SQ,
                                       B.CQ, B.lists, B.counters, B.slots, B.keys);
                else
                    hipLaunchKernelGGL(k_wf_shade, sgrid, dim3(kShadeBlock), 0, st, s->dev, R, step, B.W, B.SQ, B.CQ,
                                       (const WfClosestQ*)B.CQP, B.lists, B.counters, B.slots, B.keys);
            },
            [&](const auto& B, dim3 pgrid) {
                hipLaunchKernelGGL(k_wf_primary, pgrid, dim3(256), 0, st, s->dev, R, B.W, B.CQP, B.closest_list,
                                   B.counters + 2);
            },
            [&](const auto& B) {
                hipLaunchKernelGGL(k_wf_final, grid, dim3(256), 0, st, s->dev, R, (const WfPath*)B.W, out_dev);
            });
    }
    const dim3 rgrid((unsigned)L.blocks), rblock(kRenderBlock);
    RCCHK(launch_begin(s, st));
    if (count) HIPCHK(hipMemsetAsync(s->stats, 0, sizeof(StatsDev), st));
    s->last = pt_launch_info{PT_PATH_SINGLE, 1, (int32_t)R.split, p->flags};
    if (lens) {   // (validate: never with count)
        pt_lens_render(f64, bvh, aa, rgrid, st, s->dev, R, out_dev);
    } else if (aa) {   // (validate: never with count)
        pt_aa_render(f64, bvh, rgrid, st, s->dev, R, out_dev);
    } else {   // (forced f64, and scenes with meshes: the BVH instantiation)
        const auto k = f64   ? (count ? k_render<true, true, true> : k_render<true, false, true>)
                       : bvh ? (count ? k_render<false, true, true> : k_render<false, false, true>)
                             : (count ? k_render<false, true, false> : k_render<false, false, false>);
        hipLaunchKernelGGL(k, rgrid, rblock, 0, st, s->dev, R, out_dev, s->stats);
    }
    RCCHK(launch_end(s, st));
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        if (count) {
            StatsDev h;
            HIPCHK(hipMemcpyAsync(&h, s->stats, sizeof(h), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            stats->closest_tests = h.v[0];
            stats->shadow_tests = h.v[1];
            stats->ray_bounces = h.v[2];
            stats->shading_points = h.v[3];
            stats->light_hits = h.v[4];
            stats->escapes = h.v[5];
            stats->f64_fallbacks = h.v[6];
            stats->f64_rescans = h.v[7];
        }
    }
    return PT_OK;
}

// pt_radiance (include/pt_capi.h): on a BVH scene the wavefront kernels'
// ray form, by the frames' rule (wf_route); else, or with
// PT_FLAG_RAYS_SINGLE, one launch of k_render_rays (pt_rays.hip).
static_assert(sizeof(pt_ray) == sizeof(RayK) && offsetof(pt_ray, d) == offsetof(RayK, d) &&
                  offsetof(pt_ray, key) == offsetof(RayK, key),
              "pt_ray is the kernels' RayK");
int pt_radiance_device(pt_scene* s, const pt_ray* rays_dev, int64_t n_rays, const pt_render_params* p,
                       void* out_rgb_dev, double* out_S_dev, double* out_Q_dev, void* stream) {
    PLANCHK(check_rays(p, s != nullptr, n_rays, out_S_dev != nullptr, out_Q_dev != nullptr));
    if (n_rays == 0) return PT_OK;
    if (!rays_dev) return fail(PT_EINVAL, "null ray array");
    if (!out_rgb_dev) return fail(PT_EINVAL, "null output");
    DeviceGuard g(s->device);
    hipStream_t st = (hipStream_t)stream;
    const PlanScene ps = plan_scene(s);
    RaysK R;
    LaunchPlan L;
    PLANCHK(plan_rays(p, n_rays, ps, &R, &L));
    const RayK* rays = (const RayK*)rays_dev;
    if (L.wavefront) {
        // The ray form of render_wavefront: the loop over the slots of the
        // batch's records — a centre-ray launch with the record in the place
        // of the pixel — through the kernels of pt_shade_rays.hip for the
        // shade, primary and final steps; with S and Q (both or neither) the
        // slots' moment home as in the list form.
        // Bytes in s->wf: ~440 per slot (WfPath 256, WfShadowQ 96, WfClosestQ
        // 48, the lists, keys and sorted list 34), + 48 with S and Q, and 48
        // per record.
        const bool moments = out_S_dev != nullptr;
        const dim3 grid((unsigned)L.wf_blocks);
        const WfPass P{R.n_rays, R.split_log2, R.spp, R.bounces, false, moments};
        return render_wavefront(
            s, P, grid, st, p->flags, nullptr,
            [&](const auto& B, int32_t step, dim3 sgrid) {
                pt_wf_shade_rays(sgrid, st, s->dev, R, step, rays, B.W, B.SQ, B.CQ, (const WfClosestQ*)B.CQP, B.lists,
                                 B.counters, B.slots, B.keys, moments ? B.home : nullptr);
            },
            [&](const auto& B, dim3 pgrid) {
                pt_wf_primary_rays(pgrid, st, s->dev, R, rays, B.W, B.CQP, B.closest_list, B.counters + 2);
            },
            [&](const auto& B) {
                pt_wf_final_rays(grid, st, R, (const WfPath*)B.W, moments ? (const double*)B.home : nullptr, B.slots,
                                 out_rgb_dev, out_S_dev, out_Q_dev);
            });
    }
    RCCHK(launch_begin(s, st));
    s->last = pt_launch_info{PT_PATH_SINGLE, 1, (int32_t)R.split, p->flags};
    pt_rays_render((p->flags & PT_FLAG_FORCE_F64) != 0, ps.bvh, dim3((unsigned)L.blocks), st, s->dev, R, rays,
                   out_rgb_dev, out_S_dev, out_Q_dev);
    return launch_end(s, st);
}

int pt_radiance(pt_scene* s, const pt_ray* rays, int64_t n_rays, const pt_render_params* p, void* out_rgb,
                double* out_S, double* out_Q) {
    if (!p) return fail(PT_EINVAL, "null params");
    if (!s) return fail(PT_EINVAL, "null scene");
    if (n_rays < 0 || n_rays >= ((int64_t)1 << 30)) return fail(PT_EINVAL, "need 0 <= n_rays < 2^30");
    if (n_rays > 0 && !rays) return fail(PT_EINVAL, "null ray array");
    if (n_rays > 0 && !out_rgb) return fail(PT_EINVAL, "null output");
    for (int64_t i = 0; i < n_rays; ++i)
        if (rays[i].reserved != 0) return fail(PT_EINVAL, "ray record " + std::to_string(i) + ": reserved must be 0");
    if ((out_S == nullptr) != (out_Q == nullptr)) return fail(PT_EINVAL, "out_S and out_Q: both or neither");
    DeviceGuard g(s->device);
    const bool mom = out_S != nullptr;
    const size_t n = (size_t)n_rays;
    const size_t elem = (p->flags & PT_FLAG_OUT_F64) ? sizeof(double) : sizeof(float);
    // one staging block: the records, the means, S and Q (256-byte aligned sections)
    const size_t b_rays = align_up(n * sizeof(pt_ray)), b_rgb = align_up(n * 3 * elem), b_m = align_up(n * 3 * sizeof(double));
    char* blk = nullptr;
    if (n > 0) HIPCHK(hipMalloc((void**)&blk, b_rays + b_rgb + 2 * b_m));
    int rc = PT_OK;
    if (n > 0 && hipMemcpyAsync(blk, rays, n * sizeof(pt_ray), hipMemcpyHostToDevice, s->stream) != hipSuccess)
        rc = fail(PT_EHIP, "hipMemcpy ray records");
    double* dS = mom && blk ? (double*)(blk + b_rays + b_rgb) : nullptr;
    double* dQ = mom && blk ? (double*)(blk + b_rays + b_rgb + b_m) : nullptr;
    // (n_rays = 0: the device form checks the parameters and launches nothing)
    if (rc == PT_OK)
        rc = pt_radiance_device(s, (const pt_ray*)blk, n_rays, p, blk ? (void*)(blk + b_rays) : nullptr, dS, dQ,
                                s->stream);
    if (rc == PT_OK && n > 0) {
        if (hipMemcpyAsync(out_rgb, blk + b_rays, n * 3 * elem, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
            (mom && (hipMemcpyAsync(out_S, dS, n * 3 * sizeof(double), hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
                     hipMemcpyAsync(out_Q, dQ, n * 3 * sizeof(double), hipMemcpyDeviceToHost, s->stream) != hipSuccess)) ||
            hipStreamSynchronize(s->stream) != hipSuccess)
            rc = fail(PT_EHIP, "copying the results back");
    }
    if (blk) {
        (void)hipStreamSynchronize(s->stream);
        (void)hipFree(blk);
    }
    return rc;
}

int pt_render(pt_scene* s, const pt_render_params* p, void* out_host, pt_stats* stats) {
    PLANCHK(validate(p));
    if (!s) return fail(PT_EINVAL, "null scene");
    int32_t first = 0, rows = 0;
    band_layout(p, &first, &rows);
    if (rows == 0) return PT_OK;
    if (!out_host) return fail(PT_EINVAL, "null output");
    DeviceGuard g(s->device);
    const size_t elem = (p->flags & PT_FLAG_OUT_F64) ? sizeof(double) : sizeof(float);
    const size_t row_bytes = (size_t)p->width * 3 * elem;
    const size_t bytes = (size_t)rows * row_bytes;
    if (bytes > s->out_cap) {
        if (s->out_dev) (void)hipFree(s->out_dev);
        s->out_dev = nullptr;
        s->out_cap = 0;
        HIPCHK(hipMalloc(&s->out_dev, bytes));
        s->out_cap = bytes;
    }
    pt_render_params q = *p;   // packed in the staging buffer, strided on the host
    q.out_row_stride = 0;
    RCCHK(pt_render_device(s, &q, s->out_dev, s->stream, stats));
    if (p->out_row_stride == 0 || (size_t)p->out_row_stride * elem == row_bytes)
        HIPCHK(hipMemcpyAsync(out_host, s->out_dev, bytes, hipMemcpyDeviceToHost, s->stream));
    else
        HIPCHK(hipMemcpy2DAsync(out_host, (size_t)p->out_row_stride * elem, s->out_dev, row_bytes,
                                row_bytes, (size_t)rows, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return PT_OK;
}

}  // extern "C"

// ------------------------------------------------ pt_accum (adaptive) --
struct pt_accum {
    pt_scene* scene = nullptr;
    int32_t W = 0, H = 0;
    uint32_t npix = 0, nblocks = 0;   // nblocks: k_accum_select_*'s grid
    double *S = nullptr, *Q = nullptr, *err = nullptr;
    uint32_t *n = nullptr, *list = nullptr, *bcount = nullptr;
    AccumMeta* meta = nullptr;
    double* home = nullptr;           // k_render_list's moment home, grown on demand
    uint64_t home_lanes = 0;
    hipStream_t stream = nullptr;     // the synchronous reads
    // the last select's result, while the accumulator is unchanged since
    bool list_valid = false;
    AccumMeta list_meta{};
    pt_adapt_params list_params{};
    // denoising (pt_accum_features / pt_accum_denoise_device), allocated at
    // first use: the first-hit features and the filter's two (c, v) frames
    int32_t *f_tri = nullptr, *f_obj = nullptr;
    double *f_N = nullptr, *f_P = nullptr;
    bool features_valid = false;
    double* dn[4] = {nullptr, nullptr, nullptr, nullptr};   // c, v of frame A; c, v of frame B
    // the band the select works on (pt_accum_set_band; default: the whole
    // frame, whose select is the whole-frame kernels') and the fixed lanes
    // per pixel of a pass (0: choose_split)
    BandK band{};
    bool whole = true;
    uint32_t lanes_per_pixel = 0;
    // PT_FLAG_AA of the passes since the last reset, write or import (-1: none
    // yet): a pass with the other value is refused
    int aa = -1;
    int lens = -1;   // PT_FLAG_LENS likewise
    // a ray accumulator (pt_accum_create_rays): its own copy of the W*H
    // records, element e's primary ray; null: a frame accumulator
    RayK* rays = nullptr;
};

// pt_accum_band -> BandK, or PT_EINVAL
static int check_band(const pt_accum* a, const pt_accum_band* b, BandK* B) {
    if (!b) return fail(PT_EINVAL, "null band");
    if (b->row_step < 1) return fail(PT_EINVAL, "band: row_step must be >= 1");
    if (b->row_phase < 0 || b->row_phase >= b->row_step) return fail(PT_EINVAL, "band: need 0 <= row_phase < row_step");
    if (b->row_begin < 0 || b->row_end > a->H || b->row_begin > b->row_end)
        return fail(PT_EINVAL, "band: need 0 <= row_begin <= row_end <= height");
    if (!lanes_ok(b->lanes_per_pixel, 64)) return fail(PT_EINVAL, "band: lanes_per_pixel must be 0 or a power of two <= 64");
    if (b->reserved != 0) return fail(PT_EINVAL, "band: reserved must be 0");
    *B = band_make(a->W, a->H, b->row_begin, b->row_end, b->row_step, b->row_phase);
    return PT_OK;
}
static int check_whole(const pt_accum* a, const char* what) {
    if (a->whole) return PT_OK;
    return fail(PT_EINVAL, std::string(what) + " needs the whole frame: the accumulator's band leaves rows empty "
                                               "(pt_accum_set_band with the default band first)");
}

// (check_adapt: pt_plan.h)
static bool same_adapt(const pt_adapt_params& x, const pt_adapt_params& y) {
    return x.tol == y.tol && x.floor == y.floor && x.min_spp == y.min_spp && x.max_spp == y.max_spp &&
           x.step_spp == y.step_spp;
}
static PlanAccum plan_accum(const pt_accum* a) {
    return PlanAccum{a->W, a->H, a->npix, a->lanes_per_pixel, a->rays != nullptr, a->aa, a->lens};
}
// a pass changes n, S, Q (the last select's list is stale), and the
// accumulator remembers the pass's PT_FLAG_AA and PT_FLAG_LENS
static void accum_touch(pt_accum* a, bool aa, bool lens) {
    a->list_valid = false;
    a->aa = aa ? 1 : 0;
    a->lens = lens ? 1 : 0;
}

extern "C" {

void pt_accum_destroy(pt_accum* a) {
    if (!a) return;
    {
        DeviceGuard g(a->scene->device);
        if (a->stream) (void)hipStreamSynchronize(a->stream);
        void* bufs[] = {a->S, a->Q, a->err, a->n, a->list, a->bcount, a->meta, a->home,
                        a->f_tri, a->f_obj, a->f_N, a->f_P, a->dn[0], a->dn[1], a->dn[2], a->dn[3], a->rays};
        for (void* b : bufs)
            if (b) (void)hipFree(b);
        if (a->stream) (void)hipStreamDestroy(a->stream);
    }
    delete a;
}

int pt_accum_reset(pt_accum* a, void* stream) {
    if (!a) return fail(PT_EINVAL, "null accumulator");
    DeviceGuard g(a->scene->device);
    hipStream_t st = (hipStream_t)stream;
    RCCHK(launch_begin(a->scene, st));
    a->list_valid = false;
    a->list_meta = AccumMeta{};
    a->aa = -1;
    a->lens = -1;
    HIPCHK(hipMemsetAsync(a->S, 0, (size_t)a->npix * 3 * sizeof(double), st));
    HIPCHK(hipMemsetAsync(a->Q, 0, (size_t)a->npix * 3 * sizeof(double), st));
    HIPCHK(hipMemsetAsync(a->n, 0, (size_t)a->npix * sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(a->meta, 0, sizeof(AccumMeta), st));
    hipLaunchKernelGGL(k_accum_reset, dim3((a->npix + 255u) / 256u), dim3(256), 0, st, a->err, a->npix);
    return launch_end(a->scene, st);
}

// rays_dev: null for a frame accumulator, else the width*height records of a
// ray accumulator in device memory, copied here
static int accum_create(pt_scene* s, int32_t width, int32_t height, const pt_ray* rays_dev, pt_accum** out) {
    DeviceGuard g(s->device);
    pt_accum* a = new pt_accum();
    a->scene = s;
    a->W = width; a->H = height;
    a->npix = (uint32_t)((int64_t)width * height);
    a->nblocks = (uint32_t)(((uint64_t)a->npix + kSelBlock - 1) / kSelBlock);
    a->band = band_make(width, height, 0, height, 1, 0);
    const size_t np = a->npix;
    const bool ok = hipMalloc((void**)&a->S, np * 3 * sizeof(double)) == hipSuccess &&
                    hipMalloc((void**)&a->Q, np * 3 * sizeof(double)) == hipSuccess &&
                    hipMalloc((void**)&a->err, np * sizeof(double)) == hipSuccess &&
                    hipMalloc((void**)&a->n, np * sizeof(uint32_t)) == hipSuccess &&
                    hipMalloc((void**)&a->list, np * sizeof(uint32_t)) == hipSuccess &&
                    hipMalloc((void**)&a->bcount, (size_t)a->nblocks * sizeof(uint32_t)) == hipSuccess &&
                    hipMalloc((void**)&a->meta, sizeof(AccumMeta)) == hipSuccess;
    if (!ok) { pt_accum_destroy(a); return fail(PT_ENOMEM, "hipMalloc accumulator"); }
    if (hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking) != hipSuccess) {
        pt_accum_destroy(a);
        return fail(PT_EHIP, "stream creation");
    }
    if (rays_dev) {   // (synchronous: the caller's buffer may go away on return)
        if (hipMalloc((void**)&a->rays, np * sizeof(RayK)) != hipSuccess) {
            pt_accum_destroy(a);
            return fail(PT_ENOMEM, "hipMalloc ray records");
        }
        if (hipMemcpyAsync(a->rays, rays_dev, np * sizeof(RayK), hipMemcpyDeviceToDevice, a->stream) != hipSuccess ||
            hipStreamSynchronize(a->stream) != hipSuccess) {
            pt_accum_destroy(a);
            return fail(PT_EHIP, "copying the ray records");
        }
    }
    int rc = pt_accum_reset(a, a->stream);
    if (rc) { pt_accum_destroy(a); return rc; }
    *out = a;
    return PT_OK;
}

int pt_accum_create(pt_scene* s, int32_t width, int32_t height, pt_accum** out) {
    if (!out) return fail(PT_EINVAL, "null output handle");
    *out = nullptr;
    if (!s) return fail(PT_EINVAL, "null scene");
    if (width <= 0 || height <= 0) return fail(PT_EINVAL, "width/height must be > 0");
    if ((int64_t)width * height >= (int64_t)1 << 32) return fail(PT_EINVAL, "image too large for 32-bit pixel keys");
    return accum_create(s, width, height, nullptr, out);
}

int pt_accum_create_rays(pt_scene* s, const pt_ray* rays_dev, int32_t width, int32_t height, pt_accum** out) {
    if (!out) return fail(PT_EINVAL, "null output handle");
    *out = nullptr;
    if (!s) return fail(PT_EINVAL, "null scene");
    if (width <= 0 || height <= 0) return fail(PT_EINVAL, "width/height must be > 0: a ray accumulator has 1 <= width*height < 2^30 records");
    if ((int64_t)width * height >= (int64_t)1 << 30)
        return fail(PT_EINVAL, "a ray accumulator has 1 <= width*height < 2^30 records");
    if (!rays_dev) return fail(PT_EINVAL, "null ray array");
    return accum_create(s, width, height, rays_dev, out);
}

int pt_accum_select(pt_accum* a, const pt_adapt_params* ap, void* stream, uint32_t* n_active,
                    uint64_t* pass_samples) {
    if (!a) return fail(PT_EINVAL, "null accumulator");
    AdaptK A;
    PLANCHK(check_adapt(ap, &A));
    DeviceGuard g(a->scene->device);
    hipStream_t st = (hipStream_t)stream;
    if (!(a->list_valid && same_adapt(a->list_params, *ap))) {
        RCCHK(launch_begin(a->scene, st));
        a->list_valid = false;
        HIPCHK(hipMemsetAsync(a->meta, 0, sizeof(AccumMeta), st));
        // the grid: the frame's blocks, or the band's (<= the frame's: bcount fits)
        const uint32_t nb = a->whole ? a->nblocks : (uint32_t)(((uint64_t)a->band.npix + kSelBlock - 1) / kSelBlock);
        const dim3 grid(nb), block(kSelBlock);
        if (a->whole) {
            hipLaunchKernelGGL(k_accum_select_count<false>, grid, block, 0, st, a->S, a->Q, a->n, a->npix, a->band,
                               A, a->err, a->bcount, a->meta);
            hipLaunchKernelGGL(k_accum_select_scan, dim3(1), dim3(1024), 0, st, a->bcount, nb, a->meta);
            hipLaunchKernelGGL(k_accum_select_scatter<false>, grid, block, 0, st, a->err, a->n, a->npix, a->band,
                               A, a->bcount, a->list);
        } else if (nb > 0) {   // (a band with no rows: nothing to launch, the zeroed meta is its select)
            hipLaunchKernelGGL(k_accum_select_count<true>, grid, block, 0, st, a->S, a->Q, a->n, a->npix, a->band,
                               A, a->err, a->bcount, a->meta);
            hipLaunchKernelGGL(k_accum_select_scan, dim3(1), dim3(1024), 0, st, a->bcount, nb, a->meta);
            hipLaunchKernelGGL(k_accum_select_scatter<true>, grid, block, 0, st, a->err, a->n, a->npix, a->band,
                               A, a->bcount, a->list);
        }
        RCCHK(launch_end(a->scene, st));
        // the pass's one host synchronisation: the list's length (with the
        // smallest k and the pass's samples, 16 bytes)
        HIPCHK(hipMemcpyAsync(&a->list_meta, a->meta, sizeof(AccumMeta), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (a->list_meta.count > a->npix) return fail(PT_EHIP, "select: list longer than the frame");
        a->list_params = *ap;
        a->list_valid = true;
    }
    if (n_active) *n_active = a->list_meta.count;
    if (pass_samples) *pass_samples = a->list_meta.ksum;
    return PT_OK;
}

int pt_accum_render(pt_accum* a, const pt_render_params* p, const pt_adapt_params* ap, void* stream) {
    return pt_accum_render_stats(a, p, ap, stream, nullptr);
}

int pt_accum_render_stats(pt_accum* a, const pt_render_params* p, const pt_adapt_params* ap, void* stream,
                          pt_stats* stats) {
    PlanAccum pa{};
    PlanScene ps{};
    if (a) {
        pa = plan_accum(a);
        ps = plan_scene(a->scene);
    }
    AdaptK A;
    PLANCHK(check_pass(p, ap, a ? &pa : nullptr, a ? &ps : nullptr, &A));
    pt_scene* s = a->scene;
    DeviceGuard g(s->device);
    hipStream_t st = (hipStream_t)stream;
    if (stats) memset(stats, 0, sizeof(*stats));
    RCCHK(pt_accum_select(a, ap, stream, nullptr, nullptr));
    const AccumMeta m = a->list_meta;
    if (m.count == 0) return PT_OK;
    const uint32_t kmin = ~m.nkmin;
    if (kmin == 0 || kmin > A.step_spp) return fail(PT_EHIP, "select: bad pass size");
    uint32_t split;
    LaunchPlan L;
    PLANCHK(plan_pass(pa, ps, p->flags, m.count, kmin, &split, &L));
    const bool f64 = (p->flags & PT_FLAG_FORCE_F64) != 0, bvh = ps.bvh;
    const bool aa = (p->flags & PT_FLAG_AA) != 0, lens = (p->flags & PT_FLAG_LENS) != 0;
    const dim3 grid((unsigned)L.blocks), block(kRenderBlock);
    const ListK R = list_record(p, pa, A, m.count, split, L);
    if (L.wavefront) {
        // The list form of render_wavefront: the loop over the slots of the
        // active list's entries, with the list kernels for the shade, primary
        // and final steps and the slots' moment home [6][slots] beside the
        // path records.  The host knows the pass's smallest k only, so the
        // steps come from the largest k the rule allows.  Every pass
        // initialises every slot it launches (k_wf_shade_list's step 0): s->wf
        // holds whatever the previous pass or render left.
        accum_touch(a, aa, lens);
        const uint32_t* list = a->list;
        const uint32_t* n = a->n;
        const WfPass P{R.n_list, R.split_log2, (int32_t)std::min(A.step_spp, A.max_spp), R.bounces, aa || lens, true};
        return render_wavefront(
            s, P, dim3((unsigned)L.wf_blocks), st, p->flags, stats,
            [&](const auto& B, int32_t step, dim3 sgrid) {
                if (lens)   // (a lens point per sample; validate: never with the stats flags)
                    pt_wf_shade_list_lens(aa, sgrid, st, s->dev, R, step, list, n, B.W, B.SQ, B.CQ, B.lists,
                                          B.counters, B.slots, B.keys, B.home);
                else if (aa)   // (the slots start their own primary queries)
                    hipLaunchKernelGGL(k_wf_shade_list_aa, sgrid, dim3(kShadeBlock), 0, st, s->dev, R, step, list, n,
                                       B.W, B.SQ, B.CQ, B.lists, B.counters, B.slots, B.keys, B.home);
                else
                    hipLaunchKernelGGL(k_wf_shade_list, sgrid, dim3(kShadeBlock), 0, st, s->dev, R, step, list, n,
                                       B.W, B.SQ, B.CQ, (const WfClosestQ*)B.CQP, B.lists, B.counters, B.slots,
                                       B.keys, B.home);
            },
            [&](const auto& B, dim3 pgrid) {
                hipLaunchKernelGGL(k_wf_primary_list, pgrid, dim3(256), 0, st, s->dev, R, list, n, B.W, B.CQP,
                                   B.closest_list, B.counters + 2);
            },
            [&](const auto& B) {
                hipLaunchKernelGGL(k_wf_final_list, dim3((unsigned)L.wf_blocks), dim3(256), 0, st, R, list,
                                   (const double*)B.home, B.slots, a->S, a->Q, a->n);
            });
    }
#if PT_MOMENT_HOME
    if (!a->rays && R.lanes > a->home_lanes) {   // (the previous pass may still read the old one: ordered by the free)
        if (a->home) HIPCHK(hipFree(a->home));
        a->home = nullptr;
        a->home_lanes = 0;
        if (hipMalloc((void**)&a->home, (size_t)R.lanes * 6 * sizeof(double)) != hipSuccess)
            return fail(PT_ENOMEM, "hipMalloc moment home");
        a->home_lanes = R.lanes;
    }
#endif
    RCCHK(launch_begin(s, st));
    accum_touch(a, aa, lens);
    s->last = pt_launch_info{PT_PATH_SINGLE, 1, (int32_t)split, p->flags};
    if (a->rays)   // the list kernel over ray records (pt_rays_list.hip), on every scene
        pt_rays_render_list(f64, bvh, grid, st, s->dev, rays_list_record(p, pa, ps, A, m.count, split), a->rays,
                            a->list, a->S, a->Q, a->n);
    else if (lens)
        pt_lens_render_list(f64, bvh, aa, grid, st, s->dev, R, a->list, a->S, a->Q, a->n);
    else if (aa)
        pt_aa_render_list(f64, bvh, grid, st, s->dev, R, a->list, a->S, a->Q, a->n);
    else
        hipLaunchKernelGGL(PT_KERNEL_F64_BVH(f64, bvh, k_render_list), grid, block, 0, st, s->dev, R, a->list, a->S,
                           a->Q, a->n, a->home);
    return launch_end(s, st);
}

int pt_accum_resolve_device(pt_accum* a, uint32_t flags, void* out_dev, void* stream) {
    if (!a) return fail(PT_EINVAL, "null accumulator");
    if (!out_dev) return fail(PT_EINVAL, "null output");
    if (flags & ~(uint32_t)PT_FLAG_OUT_F64) return fail(PT_EINVAL, "resolve takes PT_FLAG_OUT_F64 only");
    DeviceGuard g(a->scene->device);
    hipStream_t st = (hipStream_t)stream;
    RCCHK(launch_begin(a->scene, st));
    hipLaunchKernelGGL(k_accum_resolve, dim3((a->npix + 255u) / 256u), dim3(256), 0, st, a->S, a->n, a->npix,
                       (flags & PT_FLAG_OUT_F64) ? 1 : 0, out_dev);
    return launch_end(a->scene, st);
}

int pt_accum_read(pt_accum* a, double* S, double* Q, uint32_t* n, double* err, uint32_t* list,
                  uint32_t list_cap, uint32_t* list_len) {
    if (!a) return fail(PT_EINVAL, "null accumulator");
    if (list && !list_len) return fail(PT_EINVAL, "list needs list_len");
    pt_scene* s = a->scene;
    DeviceGuard g(s->device);
    hipStream_t st = a->stream;
    if (s->timed) HIPCHK(hipStreamWaitEvent(st, s->ev1, 0));
    const size_t np = a->npix;
    if (S) HIPCHK(hipMemcpyAsync(S, a->S, np * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (Q) HIPCHK(hipMemcpyAsync(Q, a->Q, np * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (n) HIPCHK(hipMemcpyAsync(n, a->n, np * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (err) HIPCHK(hipMemcpyAsync(err, a->err, np * sizeof(double), hipMemcpyDeviceToHost, st));
    AccumMeta m{};
    if (list_len) HIPCHK(hipMemcpyAsync(&m, a->meta, sizeof(m), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (list_len) {
        if (m.count > a->npix) return fail(PT_EHIP, "read: list longer than the frame");
        *list_len = m.count;
        const uint32_t take = std::min(m.count, list_cap);
        if (list && take) {
            HIPCHK(hipMemcpyAsync(list, a->list, (size_t)take * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    return PT_OK;
}

int pt_accum_set_band(pt_accum* a, const pt_accum_band* band) {
    if (!a) return fail(PT_EINVAL, "null accumulator");
    BandK B;
    RCCHK(check_band(a, band, &B));
    a->band = B;
    a->whole = B.npix == a->npix;   // every row: begin 0, end height, step 1
    a->lanes_per_pixel = (uint32_t)band->lanes_per_pixel;
    a->list_valid = false;
    a->list_meta = AccumMeta{};
    return PT_OK;
}

int pt_accum_tile_bytes(int32_t width, int32_t rows, uint64_t* bytes) {
    if (!bytes) return fail(PT_EINVAL, "null output");
    if (width <= 0 || rows < 0) return fail(PT_EINVAL, "tile: need width > 0 and rows >= 0");
    *bytes = (uint64_t)60 * (uint64_t)rows * (uint64_t)width;
    return PT_OK;
}

// the four sections of a tile of P pixels
static void tile_sections(void* tile, uint64_t P, double** tS, double** tQ, double** tE, uint32_t** tN) {
    char* t = (char*)tile;
    *tS = (double*)t;
    *tQ = (double*)(t + 24 * P);
    *tE = (double*)(t + 48 * P);
    *tN = (uint32_t*)(t + 56 * P);
}

int pt_accum_export_band_device(pt_accum* a, void* tile_dev, void* stream) {
    if (!a) return fail(PT_EINVAL, "null accumulator");
    const BandK B = a->band;
    if (B.npix == 0) return PT_OK;   // no rows: an empty tile
    if (!tile_dev || ((uintptr_t)tile_dev & 7u)) return fail(PT_EINVAL, "tile: need 8-byte aligned device memory");
    DeviceGuard g(a->scene->device);
    hipStream_t st = (hipStream_t)stream;
    RCCHK(launch_begin(a->scene, st));
    double *tS, *tQ, *tE;
    uint32_t* tN;
    tile_sections(tile_dev, B.npix, &tS, &tQ, &tE, &tN);
    const uint64_t blocks = (3u * (uint64_t)B.npix + 255u) / 256u;
    hipLaunchKernelGGL(k_accum_export_band, dim3((unsigned)blocks), dim3(256), 0, st, a->S, a->Q, a->err, a->n, B,
                       tS, tQ, tE, tN);
    return launch_end(a->scene, st);
}

int pt_accum_import_band_device(pt_accum* a, const pt_accum_band* band, const void* tile_dev, void* stream) {
    if (!a) return fail(PT_EINVAL, "null accumulator");
    BandK B;
    RCCHK(check_band(a, band, &B));
    if (B.npix == 0) return PT_OK;
    if (!tile_dev || ((uintptr_t)tile_dev & 7u)) return fail(PT_EINVAL, "tile: need 8-byte aligned device memory");
    DeviceGuard g(a->scene->device);
    hipStream_t st = (hipStream_t)stream;
    RCCHK(launch_begin(a->scene, st));
    a->list_valid = false;   // n, S, Q change
    a->list_meta = AccumMeta{};
    a->aa = -1;              // (the caller vouches for the tile's samples)
    a->lens = -1;
    double *tS, *tQ, *tE;
    uint32_t* tN;
    tile_sections(const_cast<void*>(tile_dev), B.npix, &tS, &tQ, &tE, &tN);
    const uint64_t blocks = (3u * (uint64_t)B.npix + 255u) / 256u;
    hipLaunchKernelGGL(k_accum_import_band, dim3((unsigned)blocks), dim3(256), 0, st, tS, tQ, tE, tN, B, a->S, a->Q,
                       a->err, a->n);
    return launch_end(a->scene, st);
}

int pt_accum_write(pt_accum* a, const double* S, const double* Q, const uint32_t* n) {
    if (!a) return fail(PT_EINVAL, "null accumulator");
    if (!S || !Q || !n) return fail(PT_EINVAL, "write needs S, Q and n");
    DeviceGuard g(a->scene->device);
    hipStream_t st = a->stream;
    RCCHK(launch_begin(a->scene, st));
    a->list_valid = false;
    a->list_meta = AccumMeta{};
    a->aa = -1;   // (the caller vouches for the state it writes)
    a->lens = -1;
    const size_t np = a->npix;
    HIPCHK(hipMemcpyAsync(a->S, S, np * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(a->Q, Q, np * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(a->n, n, np * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(a->meta, 0, sizeof(AccumMeta), st));
    hipLaunchKernelGGL(k_accum_reset, dim3((a->npix + 255u) / 256u), dim3(256), 0, st, a->err, a->npix);
    RCCHK(launch_end(a->scene, st));
    HIPCHK(hipStreamSynchronize(st));
    return PT_OK;
}

}  // extern "C"

// ------------------------------------------------------------ denoise --
static int check_denoise(const pt_denoise_params* d, DenoiseK* K) {
    if (!d) return fail(PT_EINVAL, "null denoise params");
    if (d->iters < 1 || d->iters > 8) return fail(PT_EINVAL, "need 1 <= iters <= 8");
    if (d->normal_sq < 0 || d->normal_sq > 8) return fail(PT_EINVAL, "need 0 <= normal_sq <= 8");
    if (!(d->sigma_l > 0.0)) return fail(PT_EINVAL, "sigma_l must be > 0");
    if (!(d->sigma_z > 0.0)) return fail(PT_EINVAL, "sigma_z must be > 0");
    if (!(d->eps > 0.0)) return fail(PT_EINVAL, "eps must be > 0");
    if (d->reserved != 0) return fail(PT_EINVAL, "reserved must be 0");
    K->sigma_l = d->sigma_l; K->sigma_z = d->sigma_z; K->eps = d->eps;
    K->normal_sq = d->normal_sq; K->pad = 0;
    return PT_OK;
}
// pt_denoise_times: while on, a denoise records a HIP event around each of its
// launches, waits for them and keeps the times (moments when there are any,
// the iterations, the store).  Process-wide, like pt_test_fault_inject.
static std::atomic<int32_t> g_dn_times_on{0};
static std::mutex g_dn_times_mu;
static std::vector<float> g_dn_times;
namespace {
struct DnTimer {
    bool on;
    hipStream_t st;
    std::vector<hipEvent_t> ev;
    DnTimer(hipStream_t s) : on(g_dn_times_on.load() != 0), st(s) { mark(); }
    void mark() {   // an event after what was launched so far
        if (!on) return;
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
        ev.push_back(e);
        (void)hipEventRecord(e, st);
    }
    ~DnTimer() {
        if (!ev.empty() && hipEventSynchronize(ev.back()) == hipSuccess) {
            std::vector<float> t;
            for (size_t i = 1; i < ev.size(); ++i) {
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, ev[i - 1], ev[i]);
                t.push_back(ms);
            }
            std::lock_guard<std::mutex> g(g_dn_times_mu);
            g_dn_times.swap(t);
        }
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};
}  // namespace
// The iterations and the final store.  (c, v): the input frame, which may be
// frame A of `buf` (the accumulator's moments) — the first iteration then
// writes frame B; src and dst of a launch are never the same frame.
static int denoise_launch(int32_t W, int32_t H, const DenoiseK& K, int32_t iters, const double* c,
                          const double* v, const int32_t* obj, const double* N, const double* P,
                          double* const buf[4], uint32_t flags, void* out, void* out_var,
                          hipStream_t st, DnTimer* tm) {
    const uint32_t npix = (uint32_t)((int64_t)W * H);
    const dim3 grid((npix + kDnBlock - 1u) / kDnBlock), block(kDnBlock);
    int dst = c == buf[0] ? 1 : 0;
    for (int32_t i = 0; i < iters; ++i) {
        hipLaunchKernelGGL(k_denoise_iter, grid, block, 0, st, W, H, npix, (int32_t)1 << i, K, c, v, obj, N, P,
                           buf[2 * dst], buf[2 * dst + 1]);
        tm->mark();
        c = buf[2 * dst];
        v = buf[2 * dst + 1];
        dst ^= 1;
    }
    const uint64_t n3 = (uint64_t)npix * 3u;
    const dim3 sgrid((unsigned)((n3 + kDnBlock - 1u) / kDnBlock));
    if (flags & PT_FLAG_OUT_F64)
        hipLaunchKernelGGL(k_denoise_store<double>, sgrid, block, 0, st, c, v, n3, (double*)out, (double*)out_var);
    else
        hipLaunchKernelGGL(k_denoise_store<float>, sgrid, block, 0, st, c, v, n3, (float*)out, (float*)out_var);
    tm->mark();
    HIPCHK(hipGetLastError());
    return PT_OK;
}
static int check_frame(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return fail(PT_EINVAL, "need width, height > 0");
    if ((int64_t)width * height >= (int64_t)1 << 30) return fail(PT_EINVAL, "frame too large (2^30 pixels or more)");
    return PT_OK;
}
// the features of the accumulator's frame, once (launch_begin was called)
static int accum_features_launch(pt_accum* a, hipStream_t st) {
    if (a->features_valid) return PT_OK;
    const size_t np = a->npix;
    if (!a->f_tri) {
        const bool ok = hipMalloc((void**)&a->f_tri, np * sizeof(int32_t)) == hipSuccess &&
                        hipMalloc((void**)&a->f_obj, np * sizeof(int32_t)) == hipSuccess &&
                        hipMalloc((void**)&a->f_N, np * 3 * sizeof(double)) == hipSuccess &&
                        hipMalloc((void**)&a->f_P, np * 3 * sizeof(double)) == hipSuccess;
        if (!ok) {
            for (void** b : {(void**)&a->f_tri, (void**)&a->f_obj, (void**)&a->f_N, (void**)&a->f_P}) {
                if (*b) (void)hipFree(*b);
                *b = nullptr;
            }
            return fail(PT_ENOMEM, "hipMalloc features");
        }
    }
    pt_scene* s = a->scene;
    const dim3 grid((a->npix + 255u) / 256u), block(256);
    if (a->rays)   // a ray accumulator: each record's own ray (pt_rays_list.hip)
        pt_rays_features(s->dev.n_bnode > 0, st, s->dev, s->host.frame_x, a->rays, a->npix, a->f_tri, a->f_obj,
                         a->f_N, a->f_P);
    else if (s->dev.n_bnode > 0)
        hipLaunchKernelGGL((k_features<true>), grid, block, 0, st, s->dev, a->W, a->H, a->npix, a->f_tri, a->f_obj,
                           a->f_N, a->f_P);
    else
        hipLaunchKernelGGL((k_features<false>), grid, block, 0, st, s->dev, a->W, a->H, a->npix, a->f_tri, a->f_obj,
                           a->f_N, a->f_P);
    HIPCHK(hipGetLastError());
    a->features_valid = true;
    return PT_OK;
}

extern "C" {

int pt_denoise_device(int32_t width, int32_t height, const pt_denoise_params* params, const double* c,
                      const double* v, const int32_t* obj, const double* N, const double* P, uint32_t flags,
                      void* out_rgb, void* out_var, void* stream) {
    int rc = check_frame(width, height);
    if (rc) return rc;
    DenoiseK K;
    RCCHK(check_denoise(params, &K));
    if (!c || !v || !obj || !N || !P || !out_rgb) return fail(PT_EINVAL, "null buffer");
    if (flags & ~(uint32_t)PT_FLAG_OUT_F64) return fail(PT_EINVAL, "denoise takes PT_FLAG_OUT_F64 only");
    hipStream_t st = (hipStream_t)stream;
    const size_t frame = (size_t)width * height * 3 * sizeof(double);
    double* scratch = nullptr;
    // one frame pair when a single iteration never reads what it wrote
    const int frames = params->iters > 1 ? 4 : 2;
    if (hipMallocAsync((void**)&scratch, frame * frames, st) != hipSuccess)
        return fail(PT_ENOMEM, "hipMallocAsync denoise scratch");
    double* buf[4] = {scratch, scratch + frame / sizeof(double), nullptr, nullptr};
    if (frames == 4) {
        buf[2] = scratch + 2 * (frame / sizeof(double));
        buf[3] = scratch + 3 * (frame / sizeof(double));
    }
    {
        DnTimer tm(st);
        rc = denoise_launch(width, height, K, params->iters, c, v, obj, N, P, buf, flags, out_rgb, out_var, st, &tm);
    }
    const hipError_t e = hipFreeAsync(scratch, st);
    if (!rc && e != hipSuccess) rc = fail(PT_EHIP, std::string("hipFreeAsync: ") + hipGetErrorString(e));
    return rc;
}

int pt_denoise(int32_t width, int32_t height, const pt_denoise_params* params, const double* c, const double* v,
               const int32_t* obj, const double* N, const double* P, uint32_t flags, void* out_rgb,
               void* out_var) {
    int rc = check_frame(width, height);
    if (rc) return rc;
    DenoiseK K;
    RCCHK(check_denoise(params, &K));
    if (!c || !v || !obj || !N || !P || !out_rgb) return fail(PT_EINVAL, "null buffer");
    if (flags & ~(uint32_t)PT_FLAG_OUT_F64) return fail(PT_EINVAL, "denoise takes PT_FLAG_OUT_F64 only");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_ENODEV, "no HIP device");
    const size_t np = (size_t)width * height;
    const size_t out_bytes = np * 3 * ((flags & PT_FLAG_OUT_F64) ? sizeof(double) : sizeof(float));
    double *d_c = nullptr, *d_v = nullptr, *d_N = nullptr, *d_P = nullptr;
    int32_t* d_obj = nullptr;
    void *d_out = nullptr, *d_var = nullptr;
    rc = dev_alloc_copy(&d_c, c, np * 3);
    if (!rc) rc = dev_alloc_copy(&d_v, v, np * 3);
    if (!rc) rc = dev_alloc_copy(&d_N, N, np * 3);
    if (!rc) rc = dev_alloc_copy(&d_P, P, np * 3);
    if (!rc) rc = dev_alloc_copy(&d_obj, obj, np);
    if (!rc && hipMalloc(&d_out, out_bytes) != hipSuccess) rc = fail(PT_ENOMEM, "hipMalloc failed");
    if (!rc && out_var && hipMalloc(&d_var, out_bytes) != hipSuccess) rc = fail(PT_ENOMEM, "hipMalloc failed");
    if (!rc) rc = pt_denoise_device(width, height, params, d_c, d_v, d_obj, d_N, d_P, flags, d_out, d_var, nullptr);
    if (!rc) {
        hipError_t e = hipStreamSynchronize(nullptr);
        if (e == hipSuccess) e = hipMemcpy(out_rgb, d_out, out_bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess && out_var) e = hipMemcpy(out_var, d_var, out_bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(PT_EHIP, std::string("pt_denoise: ") + hipGetErrorString(e));
    }
    for (void* p : {(void*)d_c, (void*)d_v, (void*)d_N, (void*)d_P, (void*)d_obj, d_out, d_var})
        if (p) (void)hipFree(p);
    return rc;
}

int pt_denoise_times(int32_t enable, float* ms, int32_t cap, int32_t* n) {
    if (cap < 0 || (cap > 0 && !ms)) return fail(PT_EINVAL, "bad buffer");
    g_dn_times_on.store(enable ? 1 : 0);
    std::lock_guard<std::mutex> g(g_dn_times_mu);
    if (n) *n = (int32_t)g_dn_times.size();
    for (int32_t i = 0; i < cap && i < (int32_t)g_dn_times.size(); ++i) ms[i] = g_dn_times[i];
    return PT_OK;
}

int pt_accum_features(pt_accum* a, void* stream) {
    if (!a) return fail(PT_EINVAL, "null accumulator");
    if (int rw = check_whole(a, "pt_accum_features")) return rw;
    if (a->features_valid) return PT_OK;
    DeviceGuard g(a->scene->device);
    hipStream_t st = (hipStream_t)stream;
    RCCHK(launch_begin(a->scene, st));
    RCCHK(accum_features_launch(a, st));
    return launch_end(a->scene, st);
}

int pt_accum_read_features(pt_accum* a, int32_t* tri, int32_t* obj, double* N, double* P) {
    if (!a) return fail(PT_EINVAL, "null accumulator");
    if (int rw = check_whole(a, "pt_accum_read_features")) return rw;
    pt_scene* s = a->scene;
    DeviceGuard g(s->device);
    hipStream_t st = a->stream;
    RCCHK(pt_accum_features(a, st));
    if (s->timed) HIPCHK(hipStreamWaitEvent(st, s->ev1, 0));
    const size_t np = a->npix;
    if (tri) HIPCHK(hipMemcpyAsync(tri, a->f_tri, np * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (obj) HIPCHK(hipMemcpyAsync(obj, a->f_obj, np * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (N) HIPCHK(hipMemcpyAsync(N, a->f_N, np * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (P) HIPCHK(hipMemcpyAsync(P, a->f_P, np * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return PT_OK;
}

int pt_accum_denoise_device(pt_accum* a, const pt_denoise_params* params, uint32_t flags, void* out_rgb_dev,
                            void* out_var_dev, void* stream) {
    if (!a) return fail(PT_EINVAL, "null accumulator");
    if (int rw = check_whole(a, "pt_accum_denoise_device")) return rw;
    DenoiseK K;
    int rc = check_denoise(params, &K);
    if (rc) return rc;
    if (!out_rgb_dev) return fail(PT_EINVAL, "null output");
    if (flags & ~(uint32_t)PT_FLAG_OUT_F64) return fail(PT_EINVAL, "denoise takes PT_FLAG_OUT_F64 only");
    RCCHK(check_frame(a->W, a->H));
    DeviceGuard g(a->scene->device);
    hipStream_t st = (hipStream_t)stream;
    if (!a->dn[0]) {
        const size_t frame = (size_t)a->npix * 3 * sizeof(double);
        bool ok = true;
        for (int i = 0; i < 4 && ok; ++i) ok = hipMalloc((void**)&a->dn[i], frame) == hipSuccess;
        if (!ok) {
            for (int i = 0; i < 4; ++i) {
                if (a->dn[i]) (void)hipFree(a->dn[i]);
                a->dn[i] = nullptr;
            }
            return fail(PT_ENOMEM, "hipMalloc denoise scratch");
        }
    }
    RCCHK(launch_begin(a->scene, st));
    RCCHK(accum_features_launch(a, st));
    {
        DnTimer tm(st);
        hipLaunchKernelGGL(k_accum_moments, dim3((a->npix + kDnBlock - 1u) / kDnBlock), dim3(kDnBlock), 0, st, a->S,
                           a->Q, a->n, a->npix, a->dn[0], a->dn[1]);
        tm.mark();
        rc = denoise_launch(a->W, a->H, K, params->iters, a->dn[0], a->dn[1], a->f_obj, a->f_N, a->f_P, a->dn,
                            flags, out_rgb_dev, out_var_dev, st, &tm);
    }
    if (rc) return rc;
    return launch_end(a->scene, st);
}

}  // extern "C"

static void add_stats(pt_stats* d, const pt_stats& s) {
    d->closest_tests += s.closest_tests; d->shadow_tests += s.shadow_tests;
    d->ray_bounces += s.ray_bounces; d->shading_points += s.shading_points;
    d->light_hits += s.light_hits; d->escapes += s.escapes;
    d->f64_fallbacks += s.f64_fallbacks; d->f64_rescans += s.f64_rescans;
    d->shadow_queries += s.shadow_queries; d->shadow_node_visits += s.shadow_node_visits;
    d->shadow_leaf_units += s.shadow_leaf_units; d->closest_queries += s.closest_queries;
    d->closest_node_visits += s.closest_node_visits; d->closest_leaf_units += s.closest_leaf_units;
    d->shade_ms += s.shade_ms; d->shadow_ms += s.shadow_ms; d->closest_ms += s.closest_ms;
    d->shade_launches += s.shade_launches; d->shadow_launches += s.shadow_launches;
    d->closest_launches += s.closest_launches;
    d->sort_ms += s.sort_ms; d->sort_launches += s.sort_launches;
}
static_assert(sizeof(pt_stats) == 19 * 8 + 3 * 8, "add_stats covers every pt_stats field");

extern "C" {

// Waits for the work already queued on the first n handles' streams (the
// error path of pt_render_multi: asynchronous band renders and copies of
// devices launched before the failing one must not outlive the call).
static void drain(pt_scene* const* scenes, int32_t n) {
    for (int32_t i = 0; i < n; ++i) {
        DeviceGuard g(scenes[i]->device);
        (void)hipStreamSynchronize(scenes[i]->stream);
    }
}

int pt_render_multi(pt_scene* const* scenes, int32_t n, const pt_render_params* p, void* out_host,
                    pt_stats* stats) {
    if (!scenes || n <= 0) return fail(PT_EINVAL, "need n >= 1 scene handles");
    for (int32_t i = 0; i < n; ++i) {
        if (!scenes[i]) return fail(PT_EINVAL, "null scene handle");
        if (scenes[i]->fingerprint != scenes[0]->fingerprint)
            return fail(PT_EINVAL, "handle " + std::to_string(i) + " holds another scene than handle 0");
    }
    PLANCHK(validate(p));
    // fault injection for the tests of the error path (pt_test_fault_inject):
    // dealing band i fails after bands 0..i-1 were launched
    const int32_t fail_at = g_fault_multi.load();
    if (p->row_step != 1) return fail(PT_EINVAL, "pt_render_multi deals out the rows itself: row_step must be 1");
    if (p->out_row_stride != 0) return fail(PT_EINVAL, "pt_render_multi writes the packed layout: out_row_stride must be 0");
    int32_t first = 0, total = 0;
    band_layout(p, &first, &total);
    if (total == 0) return PT_OK;
    if (!out_host) return fail(PT_EINVAL, "null output");
    const int32_t rb = first, re = first + total;   // the rows, clamped to the image
    const size_t elem = (p->flags & PT_FLAG_OUT_F64) ? sizeof(double) : sizeof(float);
    const size_t row_bytes = (size_t)p->width * 3 * elem;
    // any stats-producing flag: every device's pt_stats is summed field by
    // field (counts and the kernel-time sums alike)
    const bool count = (p->flags & (PT_FLAG_COUNT | PT_FLAG_WALK_COUNT | PT_FLAG_KERNEL_TIMES)) != 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    std::vector<pt_render_params> bp(n);
    std::vector<int32_t> rows(n, 0);
    // 1. every device renders its band into its staging buffer (asynchronous);
    // a failure drains the devices launched so far (and this one) first
    for (int32_t i = 0; i < n; ++i) {
        pt_scene* s = scenes[i];
        bp[i] = *p;
        bp[i].row_begin = rb;
        bp[i].row_end = re;
        bp[i].row_step = n;
        bp[i].row_phase = (rb + i) % n;
        int32_t f = 0;
        band_layout(&bp[i], &f, &rows[i]);
        if (rows[i] == 0) continue;
        int rci = PT_OK;
        {
            DeviceGuard g(s->device);
            const size_t bytes = (size_t)rows[i] * row_bytes;
            if (bytes > s->out_cap) {
                // (the handle's previous work may still read or write it)
                if (hipStreamSynchronize(s->stream) != hipSuccess) {
                    rci = fail(PT_EHIP, "hipStreamSynchronize before growing a staging buffer failed");
                } else {
                    if (s->out_dev) (void)hipFree(s->out_dev);
                    s->out_dev = nullptr;
                    s->out_cap = 0;
                    if (hipMalloc(&s->out_dev, bytes) != hipSuccess)
                        rci = fail(PT_ENOMEM, "hipMalloc band staging buffer");
                    else
                        s->out_cap = bytes;
                }
            }
            if (rci == PT_OK && i == fail_at) rci = fail(PT_EHIP, "fault injected (pt_test_fault_inject)");
            if (rci == PT_OK) {
                pt_stats st;
                rci = pt_render_device(s, &bp[i], s->out_dev, s->stream, (count && stats) ? &st : nullptr);
                if (rci == PT_OK && count && stats) add_stats(stats, st);
            }
        }
        if (rci != PT_OK) {
            const std::string msg = g_err;
            drain(scenes, i + 1);
            g_err = "device " + std::to_string(i) + ": " + msg;
            return rci;
        }
    }
    // 2. each band lands in its rows of the host frame: band row j (launch
    // order, highest iy first) is frame row (re-1-iy) = (re-1-iy_top) + j*n
    for (int32_t i = 0; i < n; ++i) {
        if (rows[i] == 0) continue;
        pt_scene* s = scenes[i];
        DeviceGuard g(s->device);
        const int32_t phase = bp[i].row_phase;
        int32_t iy_top = re - 1;
        while (((iy_top % n) + n) % n != phase) --iy_top;
        char* dst = (char*)out_host + (size_t)(re - 1 - iy_top) * row_bytes;
        if (hipMemcpy2DAsync(dst, (size_t)n * row_bytes, s->out_dev, row_bytes, row_bytes, (size_t)rows[i],
                             hipMemcpyDeviceToHost, s->stream) != hipSuccess) {
            drain(scenes, n);
            return fail(PT_EHIP, "hipMemcpy2DAsync of device " + std::to_string(i) + "'s band failed");
        }
    }
    int rc_sync = PT_OK;
    for (int32_t i = 0; i < n; ++i) {
        DeviceGuard g(scenes[i]->device);
        if (hipStreamSynchronize(scenes[i]->stream) != hipSuccess && rc_sync == PT_OK)
            rc_sync = fail(PT_EHIP, "hipStreamSynchronize of device " + std::to_string(i) + " failed");
    }
    return rc_sync;
}

int pt_host_map(void* host, uint64_t bytes, void** dev_ptr) {
    if (!host || !dev_ptr || bytes == 0) return fail(PT_EINVAL, "need host, bytes > 0 and dev_ptr");
    *dev_ptr = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PT_ENODEV, "no HIP device visible (the MI355X path needs a gfx950 GPU)");
    HIPCHK(hipHostRegister(host, (size_t)bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    void* d = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&d, host, 0);
    if (e != hipSuccess) {
        (void)hipHostUnregister(host);
        return fail(PT_EHIP, std::string("hipHostGetDevicePointer failed: ") + hipGetErrorString(e));
    }
    *dev_ptr = d;
    return PT_OK;
}

int pt_host_unmap(void* host) {
    if (!host) return fail(PT_EINVAL, "null host pointer");
    HIPCHK(hipHostUnregister(host));
    return PT_OK;
}

int pt_signal(uint64_t* flag_dev, uint64_t value, void* stream) {
    if (!flag_dev || ((uintptr_t)flag_dev & 7u)) return fail(PT_EINVAL, "need an 8-byte aligned flag");
    hipLaunchKernelGGL(k_signal, dim3(1), dim3(64), 0, (hipStream_t)stream, flag_dev, value);
    HIPCHK(hipGetLastError());
    return PT_OK;
}

int pt_wait_flags(const uint64_t* flags, int32_t n, int32_t stride, uint64_t value, double timeout_s) {
    if (!flags || n < 0 || stride <= 0) return fail(PT_EINVAL, "need flags, n >= 0, stride > 0");
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; ++spin) {
        int32_t i = 0;
        while (i < n && __atomic_load_n(&flags[(size_t)i * stride], __ATOMIC_RELAXED) >= value) ++i;
        if (i == n) break;
        if ((spin & 1023u) == 1023u &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
            return fail(PT_ETIMEOUT, "pt_wait_flags: flag " + std::to_string(i) + " below " +
                                         std::to_string(value) + " after " + std::to_string(timeout_s) + " s");
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return PT_OK;
}

int pt_last_launch_info(pt_scene* s, pt_launch_info* info) {
    if (!s || !info) return fail(PT_EINVAL, "null argument");
    *info = s->last;   // (PT_PATH_NONE before the first launch)
    return PT_OK;
}

int pt_last_kernel_ms(pt_scene* s, float* ms) {
    if (!s || !ms) return fail(PT_EINVAL, "null argument");
    if (!s->timed) return fail(PT_EINVAL, "no launch recorded yet");
    DeviceGuard g(s->device);
    HIPCHK(hipEventSynchronize(s->ev1));
    HIPCHK(hipEventElapsedTime(ms, s->ev0, s->ev1));
    return PT_OK;
}

int pt_image_u8_device(const void* fb_dev, int32_t width, int32_t height, uint32_t flags,
                       void* out_u8_dev, void* stream) {
    if (!fb_dev || !out_u8_dev) return fail(PT_EINVAL, "null buffer");
    if (width <= 0 || height <= 0) return fail(PT_EINVAL, "need width, height > 0");
    const int64_t n = (int64_t)width * height * 3;
    hipStream_t st = (hipStream_t)stream;
#ifndef PT_IMAGE_V2
#define PT_IMAGE_V2 1
#endif
    if (PT_IMAGE_V2) {   // pt_image.h: per-block partials, no atomics and no fills
        const int vec = ((uintptr_t)fb_dev % 16 == 0) && ((uintptr_t)out_u8_dev % 4 == 0);
        const int pblocks = (int)std::max<int64_t>(1, std::min<int64_t>((n / 4 + 255) / 256, kImgBlocks));
#ifndef PT_IMG_U8_BLOCKS
#define PT_IMG_U8_BLOCKS 2048
#endif
        const int ublocks = (int)std::max<int64_t>(1, std::min<int64_t>((n / 16 + 255) / 256, PT_IMG_U8_BLOCKS));
        double* part = nullptr;
        HIPCHK(hipMallocAsync((void**)&part, 2 * sizeof(double) * (size_t)pblocks, st));
        if (flags & PT_FLAG_OUT_F64) {
            hipLaunchKernelGGL(k_minmax2<double>, dim3(pblocks), dim3(256), 0, st, (const double*)fb_dev, n, vec,
                               part);
            hipLaunchKernelGGL(k_to_u8_2<double>, dim3(ublocks), dim3(256), 0, st, (const double*)fb_dev, n, vec,
                               part, pblocks, (uint8_t*)out_u8_dev);
        } else {
            hipLaunchKernelGGL(k_minmax2<float>, dim3(pblocks), dim3(256), 0, st, (const float*)fb_dev, n, vec,
                               part);
            hipLaunchKernelGGL(k_to_u8_2<float>, dim3(ublocks), dim3(256), 0, st, (const float*)fb_dev, n, vec,
                               part, pblocks, (uint8_t*)out_u8_dev);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipFreeAsync(part, st));
        return PT_OK;
    }
    unsigned long long* keys = nullptr;
    HIPCHK(hipMallocAsync((void**)&keys, 2 * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(keys, 0xff, sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(keys + 1, 0, sizeof(unsigned long long), st));
    // 4 elements per thread step when the buffers allow 16-byte loads and
    // 4-byte stores; ~8 blocks per CU of grid-stride work
    const int vec = ((uintptr_t)fb_dev % 16 == 0) && ((uintptr_t)out_u8_dev % 4 == 0);
    const int blocks = (int)std::min<int64_t>((n / 4 + 255) / 256 + 1, 2048);
    if (flags & PT_FLAG_OUT_F64) {
        hipLaunchKernelGGL(k_minmax<double>, dim3(blocks), dim3(256), 0, st, (const double*)fb_dev, n, vec, keys);
        hipLaunchKernelGGL(k_to_u8<double>, dim3(blocks), dim3(256), 0, st, (const double*)fb_dev, n, vec, keys,
                           (uint8_t*)out_u8_dev);
    } else {
        hipLaunchKernelGGL(k_minmax<float>, dim3(blocks), dim3(256), 0, st, (const float*)fb_dev, n, vec, keys);
        hipLaunchKernelGGL(k_to_u8<float>, dim3(blocks), dim3(256), 0, st, (const float*)fb_dev, n, vec, keys,
                           (uint8_t*)out_u8_dev);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipFreeAsync(keys, st));
    return PT_OK;
}

int pt_assemble_bands_device(const void* tiles_dev, int32_t world, int32_t max_rows, int32_t width,
                             int32_t height, uint32_t flags, void* out_dev, void* stream) {
    if (!tiles_dev || !out_dev) return fail(PT_EINVAL, "null buffer");
    if (world <= 0 || width <= 0 || height <= 0) return fail(PT_EINVAL, "need world, width, height > 0");
    if (max_rows < (height + world - 1) / world)
        return fail(PT_EINVAL, "max_rows is smaller than the largest band (ceil(height / world))");
    const int64_t row_bytes = (int64_t)width * 3 * ((flags & PT_FLAG_OUT_F64) ? 8 : 4);
    const bool v16 = row_bytes % 16 == 0 && (uintptr_t)tiles_dev % 16 == 0 && (uintptr_t)out_dev % 16 == 0;
    const int64_t units = row_bytes / (v16 ? 16 : 4);
    const int64_t n = (int64_t)height * units;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (v16)
        hipLaunchKernelGGL(k_assemble_bands<uint4>, grid, block, 0, st, (const uint4*)tiles_dev, world, max_rows,
                           height, units, (uint4*)out_dev);
    else
        hipLaunchKernelGGL(k_assemble_bands<uint32_t>, grid, block, 0, st, (const uint32_t*)tiles_dev, world,
                           max_rows, height, units, (uint32_t*)out_dev);
    HIPCHK(hipGetLastError());
    return PT_OK;
}

int pt_image_u8(const void* fb_host, int32_t width, int32_t height, uint32_t flags,
                uint8_t* out_u8_host) {
    if (!fb_host || !out_u8_host) return fail(PT_EINVAL, "null buffer");
    if (width <= 0 || height <= 0) return fail(PT_EINVAL, "need width, height > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PT_ENODEV, "no HIP device");
    const size_t n = (size_t)width * height * 3;
    const size_t in_bytes = n * ((flags & PT_FLAG_OUT_F64) ? sizeof(double) : sizeof(float));
    void *d_in = nullptr, *d_out = nullptr;
    HIPCHK(hipMalloc(&d_in, in_bytes));
    if (hipMalloc(&d_out, n) != hipSuccess) {
        (void)hipFree(d_in);
        return fail(PT_ENOMEM, "hipMalloc failed");
    }
    int rc = PT_OK;
    if (hipMemcpy(d_in, fb_host, in_bytes, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(PT_EHIP, "hipMemcpy to device failed");
    if (!rc) rc = pt_image_u8_device(d_in, width, height, flags, d_out, nullptr);
    if (!rc && hipMemcpy(out_u8_host, d_out, n, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(PT_EHIP, "hipMemcpy to host failed");
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}

struct pt_mesh_impl {
    pt_mesh pub;
    MeshOut data;
};

int pt_obj_load(const char* path, pt_mesh** out) {
    if (!path || !out) return fail(PT_EINVAL, "null argument");
    *out = nullptr;
    pt_mesh_impl* m = new (std::nothrow) pt_mesh_impl();
    if (!m) return fail(PT_ENOMEM, "out of host memory");
    int rc;
    try {
        rc = parse_obj_file(path, &m->data);
    } catch (const std::bad_alloc&) {
        delete m;
        return fail(PT_ENOMEM, "out of host memory");
    }
    if (rc != kIngestOk) {
        delete m;
        if (rc == kIngestIo) return fail(PT_EINVAL, std::string("cannot read ") + path);
        return fail(PT_EUNSUPPORTED, rc == kIngestDivZero
                                         ? "zero-area triangle (the reference divides by zero)"
                                         : "input outside the fast reader's subset");
    }
    const MeshOut& d = m->data;
    m->pub.n_vert = (int64_t)(d.vert.size() / 3);
    m->pub.n_tri = (int64_t)d.tri_area.size();
    m->pub.n_skip = (int64_t)d.skip_off.size();
    m->pub.vert = d.vert.data();
    m->pub.face = d.face.data();
    m->pub.tri_v = d.tri_v.data();
    m->pub.tri_n = d.tri_n.data();
    m->pub.tri_area = d.tri_area.data();
    m->pub.skip_off = d.skip_off.data();
    m->pub.skip_len = d.skip_len.data();
    *out = &m->pub;
    return PT_OK;
}

void pt_mesh_free(pt_mesh* m) {
    delete reinterpret_cast<pt_mesh_impl*>(m);   // pub is the first member
}

int pt_intersect_objects(pt_scene* s, const double* rays, int64_t n, int32_t* out_tri,
                         double* out_p) {
    if (!s || (n > 0 && (!rays || !out_tri || !out_p))) return fail(PT_EINVAL, "null argument");
    if (n <= 0) return PT_OK;
    DeviceGuard g(s->device);
    double *d_rays = nullptr, *d_p = nullptr;
    int32_t* d_tri = nullptr;
    int rc = dev_alloc_copy(&d_rays, rays, (size_t)n * 6);
    if (!rc) rc = dev_alloc_copy(&d_p, (const double*)nullptr, (size_t)n * 3);
    if (!rc) rc = dev_alloc_copy(&d_tri, (const int32_t*)nullptr, (size_t)n);
    if (!rc) {
        hipLaunchKernelGGL(k_intersect, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream,
                           s->dev, d_rays, n, s->xb_surf, s->xb_all, d_tri, d_p);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e == hipSuccess) e = hipMemcpy(out_tri, d_tri, n * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(out_p, d_p, n * 3 * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(PT_EHIP, std::string("k_intersect: ") + hipGetErrorString(e));
    }
    if (d_rays) (void)hipFree(d_rays);
    if (d_p) (void)hipFree(d_p);
    if (d_tri) (void)hipFree(d_tri);
    return rc;
}

int pt_compute_color(pt_scene* s, const int32_t* obj, const double* point, const double* normal,
                     const double* u, int64_t n, double* out_rgb) {
    if (!s || (n > 0 && (!obj || !point || !normal || !u || !out_rgb)))
        return fail(PT_EINVAL, "null argument");
    if (n <= 0) return PT_OK;
    for (int64_t i = 0; i < n; ++i)
        if (obj[i] < 0 || obj[i] >= s->host.k.n_obj) return fail(PT_EINVAL, "object index out of range");
    DeviceGuard g(s->device);
    int32_t* d_obj = nullptr;
    double *d_pt = nullptr, *d_n = nullptr, *d_u = nullptr, *d_out = nullptr;
    int rc = dev_alloc_copy(&d_obj, obj, (size_t)n);
    if (!rc) rc = dev_alloc_copy(&d_pt, point, (size_t)n * 3);
    if (!rc) rc = dev_alloc_copy(&d_n, normal, (size_t)n * 3);
    if (!rc) rc = dev_alloc_copy(&d_u, u, (size_t)n * 12);
    if (!rc) rc = dev_alloc_copy(&d_out, (const double*)nullptr, (size_t)n * 3);
    if (!rc) {
        hipLaunchKernelGGL(k_color, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream,
                           s->dev, d_obj, d_pt, d_n, d_u, n, s->xb_surf, s->xb_all, d_out);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e == hipSuccess) e = hipMemcpy(out_rgb, d_out, n * 3 * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(PT_EHIP, std::string("k_color: ") + hipGetErrorString(e));
    }
    for (void* p : {(void*)d_obj, (void*)d_pt, (void*)d_n, (void*)d_u, (void*)d_out})
        if (p) (void)hipFree(p);
    return rc;
}

}  // extern "C"
