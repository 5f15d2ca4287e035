// match.hip -- the kernels of the template-correlation accumulator (include/iqgpu.h "template correlation"; host side match.cpp;
// DESIGN 3.14).
//   k_match_segs  one workgroup of nfft / 16 threads per SEGMENT of the stream's grid at hop = V = nfft / 2.  16 points a thread from the
//                 logical stream (the carry, then the pushed buffer) through psd_unpack at gain 1, no window; fft16_lds leaves the
//                 spectrum X in registers in natural order, point tid + r nfft / 16 in xs[r], and there it stays across the templates.
//                 Per template t: io[r] = conj(X G_t), fft16_lds again -- the forward transform of a conjugate is the conjugate of the
//                 inverse one, and G_t carries the 1 / nfft -- so |io[r]|^2 = p_t[s V + tid + r nfft / 16].  Only r < 8 lies below V.
//                 A thread folds its eight powers in r order (sum in double; a power replaces the held peak only where it is greater),
//                 the wave in six levels of pairs 1, 2, 4, 8, 16, 32 lanes apart (pair_tree.hpp), the waves of the workgroup through
//                 LDS in wave order, and one thread per template stores the record to its slab slot.  No atomics.
//   k_match_fold  one thread per (row, template): the row's records in segment order behind the open record, into the caller's planes
//                 or the other open buffer.
// Ordering: the argument of psd.hip.  Within a launch every address is read only or written by exactly one workgroup (its slab
// slots) or thread (the fold); the open record is two buffers, and the host flips cur behind every launch.
#include <hip/hip_runtime.h>

#include "fft16.hpp"
#include "match.hpp"
#include "pair_tree.hpp"
#include "psd_stream.hpp"

namespace iqgpu {

// the better of two (peak, position) pairs: the greater peak, the lower position on a tie
__device__ __forceinline__ void match_best(float &m, uint32_t &n, float om, uint32_t on)
{
    const bool take = om > m || (om == m && on < n);
    m = take ? om : m;
    n = take ? on : n;
}

// one level of the wave's tree.  pair_*<M> hands over the value of SOME lane of the partner group (the levels at 4 and 8 are mirrors),
// so every lane of a group of M must hold the same (s, m, n) going in: true because a + b == b + a bit for bit and match_best is a
// total order on finite powers.  With a NaN power the lanes' peaks may part (row_peak / row_at of such a row are unspecified); the
// sum is NaN in every lane all the same.
template <int M> __device__ __forceinline__ void match_level(double &s, float &m, uint32_t &n)
{
    const double os = pair_f64<M>(s);
    const float om = pair_f32<M>(m);
    const uint32_t on = (uint32_t)pair_i32<M>((int)n);
    s += os;
    match_best(m, n, om, on);
}

template <int LOG2N, int FMT>
__global__ __launch_bounds__((1 << LOG2N) / 16) void k_match_segs(const MatchSegsArgs a)
{
    constexpr int N = 1 << LOG2N, T = N / 16, W = T / 64;
    __shared__ cf2 X[N + (N >> 5) + 2];
    __shared__ double w_sum[kMatchMaxTemplates][W];
    __shared__ float w_peak[kMatchMaxTemplates][W];
    __shared__ uint32_t w_at[kMatchMaxTemplates][W];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x;
    if (j >= a.n_seg) return;                                       // (workgroup-uniform)

    cf2 xs[16];
    {
        const int64_t i0 = a.first + j * (int64_t)a.hop + tid;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t i = i0 + r * T;
            const bool old = i < a.split;
            xs[r] = psd_unpack<FMT>(old ? a.carry : a.raw, old ? i : i - a.split, a.fmt, 1.0f);
        }
    }
    fft16_lds<LOG2N, false>(X, a.twiddle, tid, xs);

    for (int t = 0; t < a.n_templates; ++t) {
        const cf2 *g = a.g + (int64_t)t * N + tid;
        cf2 io[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const cf2 z = cmulf(xs[r], g[r * T]);
            io[r] = cf2{z.x, -z.y};
        }
        fft16_lds<LOG2N, true>(X, a.twiddle, tid, io);
        double s = 0.0;
        float m = 0.0f;
        uint32_t n = (uint32_t)tid;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float p = __fadd_rn(__fmul_rn(io[r].x, io[r].x), __fmul_rn(io[r].y, io[r].y));
            s += (double)p;
            if (r == 0) m = p;
            else if (p > m) { m = p; n = (uint32_t)(tid + r * T); }
        }
        match_level<1>(s, m, n); match_level<2>(s, m, n); match_level<4>(s, m, n);
        match_level<8>(s, m, n); match_level<16>(s, m, n); match_level<32>(s, m, n);
        if ((tid & 63) == 0) { w_sum[t][tid >> 6] = s; w_peak[t][tid >> 6] = m; w_at[t][tid >> 6] = n; }
    }
    __syncthreads();
    if (tid < a.n_templates) {
        double s = w_sum[tid][0];
        float m = w_peak[tid][0];
        uint32_t n = w_at[tid][0];
#pragma unroll
        for (int w = 1; w < W; ++w) {
            s += w_sum[tid][w];
            match_best(m, n, w_peak[tid][w], w_at[tid][w]);
        }
        a.slab[j * a.n_templates + tid] = MatchRec{s, m, n};
    }
}

hipError_t launch_match_segs(const MatchSegsArgs &a, hipStream_t s)
{
    if (a.n_seg <= 0) return hipSuccess;
    if (a.n_seg > kMatchSlabSegments || a.n_templates < 1 || a.n_templates > kMatchMaxTemplates || a.hop * 2 != (1 << a.log2n)) return hipErrorInvalidValue;
    return psd_dispatch(a.log2n, a.fmt, [&](auto L, auto F) {
        hipLaunchKernelGGL((k_match_segs<decltype(L)::value, decltype(F)::value>), dim3((unsigned)a.n_seg), dim3((1u << decltype(L)::value) / 16), 0, s, a);
    });
}

__global__ __launch_bounds__(64) void k_match_fold(const MatchFoldArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + (int64_t)threadIdx.x;
    const int64_t j = i / a.n_templates;
    const int t = (int)(i - j * a.n_templates);
    if (j >= a.n_rows) return;
    const int64_t row = a.r0 + j;
    const bool from_open = j == 0 && a.has_open_in;
    MatchRec o = from_open ? a.open_in[t] : MatchRec{0.0, 0.0f, 0u};
    const int64_t lo = row * a.R > a.seg0 ? row * a.R : a.seg0;
    const int64_t hi = (row + 1) * a.R < a.seg_end ? (row + 1) * a.R : a.seg_end;
    const MatchRec *rec = a.slab + t;
#pragma unroll 4
    for (int64_t s = lo; s < hi; ++s) {
        const MatchRec c = rec[(s - a.seg0) * a.n_templates];
        o.sum += c.sum;
        if (c.peak > o.peak) { o.peak = c.peak; o.at = (uint32_t)((s - row * a.R) * a.V) + c.at; }
    }
    if ((row + 1) * a.R <= a.seg_end) {
        const int64_t at = j * a.n_templates + t;
        if (a.row_peak) a.row_peak[at] = o.peak;
        if (a.row_at) a.row_at[at] = o.at;
        if (a.row_sum) a.row_sum[at] = (float)o.sum;
    } else {
        a.open_out[t] = o;
    }
}

hipError_t launch_match_fold(const MatchFoldArgs &a, hipStream_t s)
{
    if (a.n_rows <= 0) return hipSuccess;
    const int64_t threads = (int64_t)a.n_rows * a.n_templates;
    hipLaunchKernelGGL(k_match_fold, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}

} // namespace iqgpu
