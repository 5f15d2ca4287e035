// stats.hip -- the kernels of the capture-statistics accumulator (include/iqgpu.h "capture statistics"; host side stats.cpp).
//   k_stats_pages  one workgroup of 256 threads per run of consecutive PAGES (kStatsPageFrames frames of the stream's grid).  A row of
//                  a page is 1024 frames: thread t takes frames 4 t .. 4 t + 3 of every row -- one 16-byte load at cs16, 8 bytes at
//                  cu8 / cs8, two 16-byte loads at cf32, through unpack_b16 / unpack_b8; rows cut by the launch's ends, addresses
//                  that are not aligned to the load and the formats decoded at run time go frame by frame through the same unpack.
//                  So the thread owns columns 4 t .. 4 t + 3 of the page and sums each in row order in double registers (5 sums x 4).
//                  Counts, extrema and the peak stay in registers per thread, the histogram goes to LDS with integer adds (integer
//                  adds commute: the counts are deterministic), in kStatsSlices copies by lane (stats.hpp: a wave whose lanes all
//                  hit one bin must not queue on one address).  A page that ends inside the launch reduces its 1024 columns in the
//                  fixed tree of adjacent pairs (in the thread, xor-shuffles 1 .. 32, the four waves through LDS) and stores five
//                  doubles; the stream's open page starts from and returns to the handle's open columns, in TWO buffers flipped behind
//                  the launch, for the reason given at the top of psd.hip.  Everything leaves the workgroup as plain stores into
//                  slots of its own.  No float atomics, no global atomics.
//   k_stats_fold   blocks 0 .. 7: totals.hist += the workgroups' histograms (64 bins a block, 16 workgroups at a time); block 8: the
//                  counts, min / max and the peak (the earlier frame of equal peaks) in a tree; block 9: sum[k] += page_sum[p][k] in page order.
#include <hip/hip_runtime.h>

#include "capture_load.hpp"
#include "stats.hpp"

namespace iqgpu {

namespace {

struct StatsLane {
    uint32_t rail_lo[2], rail_hi[2], nonfinite, finite;
    float mn[2], mx[2];
    double pk; uint64_t pkf;
};

__device__ __forceinline__ void lane_init(StatsLane &L)
{
    L.rail_lo[0] = L.rail_lo[1] = L.rail_hi[0] = L.rail_hi[1] = L.nonfinite = L.finite = 0u;
    L.mn[0] = L.mn[1] = __builtin_inff(); L.mx[0] = L.mx[1] = -__builtin_inff();
    L.pk = -1.0; L.pkf = ~(uint64_t)0;
}

// the larger peak, the earlier frame of equal ones
__device__ __forceinline__ void peak_merge(double &pk, uint64_t &pkf, double opk, uint64_t opkf)
{
    if (opk > pk || (opk == pk && opkf < pkf)) { pk = opk; pkf = opkf; }
}

// one frame into the thread's state: s = the five sums of the frame's column, H = the lane's histogram copy
template <int FMT>
__device__ __forceinline__ void take(StatsLane &L, double *s, uint32_t *H, int fmt, int ci, int cq, cf2 x, int64_t idx)
{
    int bi, bq; bool li, hi, lq, hq;
    if constexpr (FMT == IQGPU_FMT_CF32) {
        if (!(fabsf(x.x) < __builtin_inff() && fabsf(x.y) < __builtin_inff())) { ++L.nonfinite; return; }
        classify_float(x.x, bi, li, hi); classify_float(x.y, bq, lq, hq);
    } else {
        const int f = FMT >= 0 ? FMT : fmt;
        classify_code(f, ci, bi, li, hi); classify_code(f, cq, bq, lq, hq);
    }
    atomicAdd(&H[bi * kStatsSlices], 1u);
    atomicAdd(&H[(256 + bq) * kStatsSlices], 1u);
    ++L.finite;
    L.rail_lo[0] += li; L.rail_hi[0] += hi; L.rail_lo[1] += lq; L.rail_hi[1] += hq;
    L.mn[0] = fminf(L.mn[0], x.x); L.mx[0] = fmaxf(L.mx[0], x.x);
    L.mn[1] = fminf(L.mn[1], x.y); L.mx[1] = fmaxf(L.mx[1], x.y);
    const double re = (double)x.x, im = (double)x.y;
    const double rr = __dmul_rn(re, re), ii = __dmul_rn(im, im);
    const double p = __dadd_rn(rr, ii);
    if (p > L.pk) { L.pk = p; L.pkf = (uint64_t)idx; }        // (a thread's frames come in increasing index: the first stays)
    s[0] = __dadd_rn(s[0], re); s[1] = __dadd_rn(s[1], im);
    s[2] = __dadd_rn(s[2], rr); s[3] = __dadd_rn(s[3], ii);
    s[4] = __dadd_rn(s[4], __dmul_rn(re, im));
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}

} // namespace

template <int FMT>
__global__ __launch_bounds__(kStatsThreads) void k_stats_pages(const StatsPagesArgs a)
{
    constexpr int64_t P = kStatsPageFrames;
    constexpr int C = kStatsColumns, S = kStatsSlices;
    __shared__ uint32_t H[512 * S];
    __shared__ double W[4][5];
    __shared__ StatsPartial R[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 512 * S; i += kStatsThreads) H[i] = 0u;
    __syncthreads();
    uint32_t *const Hl = H + (lane & (S - 1));

    const int64_t end = a.first + a.n, page_first = a.first / P, page_last = (end - 1) / P;
    const int64_t pg0 = page_first + (int64_t)blockIdx.x * a.pages_per_group;
    const int64_t pg1 = pg0 + a.pages_per_group - 1 < page_last ? pg0 + a.pages_per_group - 1 : page_last;
    const int bps = frame_bytes(FMT >= 0 ? FMT : a.fmt);

    StatsLane L;
    lane_init(L);
    for (int64_t pg = pg0; pg <= pg1; ++pg) {
        const int64_t base = pg * P;
        const int64_t fbeg = base > a.first ? base : a.first, fend = base + P < end ? base + P : end;
        const bool from_open = base < a.first, closed = base + P <= end;
        double s[4][5];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 5; ++k) s[j][k] = from_open ? a.open_in[k * C + 4 * tid + j] : 0.0;

        const int r0 = (int)((fbeg - base) / C), r1 = (int)((fend - base + C - 1) / C);
        for (int r = r0; r < r1; ++r) {
            const int64_t i0 = base + (int64_t)r * C + 4 * tid;      // stream index of the thread's first frame of the row
            const int64_t j0 = i0 - a.first;                          // ... its index in raw
            int ci[4], cq[4]; cf2 x[4]; bool ok[4];
            bool four = false;
            if constexpr (vec_bytes<FMT>() != 0)
                four = i0 >= fbeg && i0 + 4 <= fend && (((uintptr_t)a.raw + (uintptr_t)(j0 * bps)) & (uintptr_t)(vec_bytes<FMT>() - 1)) == 0;
            if (four) {
                load_four<FMT>(a.raw, j0, ci, cq, x);
#pragma unroll
                for (int k = 0; k < 4; ++k) ok[k] = true;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    ok[k] = i0 + k >= fbeg && i0 + k < fend;
                    ci[k] = cq[k] = 0; x[k] = cf2{0.0f, 0.0f};
                    if (ok[k]) load_one<FMT>(a.raw, j0 + k, a.fmt, ci[k], cq[k], x[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) take<FMT>(L, s[k], Hl, a.fmt, ci[k], cq[k], x[k], i0 + k);
        }

        if (!closed) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 5; ++k) a.open_out[k * C + 4 * tid + j] = s[j][k];
        } else {
            // the tree of adjacent pairs over the page's 1024 columns: two levels in the thread, six across the wave, two across the waves
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                double v = __dadd_rn(__dadd_rn(s[0][k], s[1][k]), __dadd_rn(s[2][k], s[3][k]));
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) v = __dadd_rn(v, __shfl_xor(v, m));      // (both lanes of a pair hold the pair's sum)
                if (lane == 0) W[wave][k] = v;
            }
            __syncthreads();
            if (tid < 5) a.page_sum[(pg - page_first) * 5 + tid] = __dadd_rn(__dadd_rn(W[0][tid], W[1][tid]), __dadd_rn(W[2][tid], W[3][tid]));
            __syncthreads();
        }
    }

    // the order-free fields: across the wave by shuffles, across the waves through LDS
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            L.rail_lo[c] += (uint32_t)__shfl_xor((int)L.rail_lo[c], m); L.rail_hi[c] += (uint32_t)__shfl_xor((int)L.rail_hi[c], m);
            L.mn[c] = fminf(L.mn[c], __shfl_xor(L.mn[c], m)); L.mx[c] = fmaxf(L.mx[c], __shfl_xor(L.mx[c], m));
        }
        L.nonfinite += (uint32_t)__shfl_xor((int)L.nonfinite, m); L.finite += (uint32_t)__shfl_xor((int)L.finite, m);
        const double opk = __shfl_xor(L.pk, m);
        const uint64_t opkf = shfl_xor_u64(L.pkf, m);
        peak_merge(L.pk, L.pkf, opk, opkf);
    }
    if (lane == 0) {
        StatsPartial &o = R[wave];
#pragma unroll
        for (int c = 0; c < 2; ++c) { o.rail_lo[c] = L.rail_lo[c]; o.rail_hi[c] = L.rail_hi[c]; o.mn[c] = L.mn[c]; o.mx[c] = L.mx[c]; }
        o.nonfinite = L.nonfinite; o.finite = L.finite; o.pk = L.pk; o.pkf = L.pkf;
    }
    __syncthreads();
    if (tid == 0) {
        StatsPartial o = R[0];
        for (int w = 1; w < 4; ++w) {
            for (int c = 0; c < 2; ++c) {
                o.rail_lo[c] += R[w].rail_lo[c]; o.rail_hi[c] += R[w].rail_hi[c];
                o.mn[c] = fminf(o.mn[c], R[w].mn[c]); o.mx[c] = fmaxf(o.mx[c], R[w].mx[c]);
            }
            o.nonfinite += R[w].nonfinite; o.finite += R[w].finite;
            peak_merge(o.pk, o.pkf, R[w].pk, R[w].pkf);
        }
        a.part[blockIdx.x] = o;
    }
    // the histogram: bins tid and tid + 256, the copies added up
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int bin = tid + h * kStatsThreads;
        const uint4 *q = (const uint4 *)&H[bin * S];
        uint32_t n = 0;
#pragma unroll
        for (int i = 0; i < S / 4; ++i) { const uint4 v = q[i]; n += v.x + v.y + v.z + v.w; }
        a.hist[(int64_t)blockIdx.x * 512 + bin] = n;
    }
}

hipError_t launch_stats_pages(const StatsPagesArgs &a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    int groups = 0, ppg = 0;
    stats_grid(a.first, a.n, &groups, &ppg);
    const int64_t pages = (a.first + a.n - 1) / kStatsPageFrames - a.first / kStatsPageFrames + 1;
    if (a.first < 0 || pages > kStatsMaxPages || ppg != a.pages_per_group) return hipErrorInvalidValue;      // (the slab's bounds: stats.cpp cuts longer pushes)
    return page_dispatch(a.fmt, [&](auto F) { hipLaunchKernelGGL(k_stats_pages<decltype(F)::value>, dim3((unsigned)groups), dim3(kStatsThreads), 0, s, a); });
}

__global__ __launch_bounds__(1024) void k_stats_fold(const StatsFoldArgs a)
{
    // (one buffer for the two uses: a block takes one branch)
    __shared__ __attribute__((aligned(16))) unsigned char lds[kStatsMaxGroups * sizeof(StatsPartial)];
    static_assert(sizeof(lds) >= 16 * 64 * sizeof(uint64_t), "the histogram blocks' scratch fits");
    StatsPartial *const R = (StatsPartial *)lds;
    uint64_t (*const T)[64] = (uint64_t (*)[64])lds;
    const int tid = threadIdx.x;
    if (blockIdx.x < 8) {
        const int col = tid & 63, grp = tid >> 6, bin = (int)blockIdx.x * 64 + col;
        uint64_t n = 0;
        for (int g = grp; g < a.groups; g += 16) n += a.hist[(int64_t)g * 512 + bin];
        T[grp][col] = n;
        __syncthreads();
        if (tid < 64) {
            uint64_t t = a.tot->hist[bin];
            for (int g = 0; g < 16; ++g) t += T[g][col];
            a.tot->hist[bin] = t;
        }
    } else if (blockIdx.x == 8) {
        StatsPartial o;
        if (tid < a.groups) o = a.part[tid];
        else {
            o.rail_lo[0] = o.rail_lo[1] = o.rail_hi[0] = o.rail_hi[1] = o.nonfinite = o.finite = 0u;
            o.mn[0] = o.mn[1] = __builtin_inff(); o.mx[0] = o.mx[1] = -__builtin_inff(); o.pk = -1.0; o.pkf = ~(uint64_t)0;
        }
        R[tid] = o;
        __syncthreads();
        // (a launch holds at most 2^28 frames: the 32-bit counts cannot wrap)
        for (int n = kStatsMaxGroups / 2; n >= 1; n >>= 1) {
            if (tid < n) {
                StatsPartial &x = R[tid];
                const StatsPartial &y = R[tid + n];
                for (int c = 0; c < 2; ++c) {
                    x.rail_lo[c] += y.rail_lo[c]; x.rail_hi[c] += y.rail_hi[c];
                    x.mn[c] = fminf(x.mn[c], y.mn[c]); x.mx[c] = fmaxf(x.mx[c], y.mx[c]);
                }
                x.nonfinite += y.nonfinite; x.finite += y.finite;
                peak_merge(x.pk, x.pkf, y.pk, y.pkf);
            }
            __syncthreads();
        }
        if (tid == 0) {
            StatsTotals &t = *a.tot;
            const StatsPartial &x = R[0];
            for (int c = 0; c < 2; ++c) {
                t.rail_lo[c] += x.rail_lo[c]; t.rail_hi[c] += x.rail_hi[c];
                t.mn[c] = fminf(t.mn[c], x.mn[c]); t.mx[c] = fmaxf(t.mx[c], x.mx[c]);
            }
            t.nonfinite += x.nonfinite; t.finite += x.finite;
            if (x.pk > t.pk) { t.pk = x.pk; t.pkf = x.pkf; }         // (the launch's frames lie behind the totals': a tie keeps the totals')
        }
    } else if (tid < 5) {
        double t = a.tot->sum[tid];
        const double *ps = a.page_sum + tid;
#pragma unroll 8
        for (int p = 0; p < a.n_pages; ++p) t = __dadd_rn(t, ps[(int64_t)p * 5]);
        a.tot->sum[tid] = t;
    }
}

hipError_t launch_stats_fold(const StatsFoldArgs &a, hipStream_t s)
{
    if (a.groups <= 0 || a.groups > kStatsMaxGroups) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_stats_fold, dim3(10), dim3(1024), 0, s, a);
    return hipGetLastError();
}

} // namespace iqgpu
