// kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the I/Q chain.
//
//   k_front      raw -> unpack/gain -> dc block -> iq correct -> NCO -> half-band cascade ->
//                256-arm polyphase -> post NCO -> pack           (one launch per process() call)
//   k_dc_prefix  per-segment aggregate of the DC blocker's first-order recurrence
//   k_dc_scan    carries of the (few) segments
//   k_fir        time-domain FIR with LDS tap tiling over the cf32 filter-input buffer
//
// Reference semantics and file:line citations are in DESIGN.md; the per-operator arithmetic
// follows sample_convert.c (bit-exact: this file is compiled with -ffp-contract=off, so a*b+c is
// two roundings unless written as fmaf(); HIP's __fmul_rn/__fadd_rn are plain operators),
// frequency_shift.c / dc_block.c / iq_correct.c / resampler.c / filter.c call sites.
#include <hip/hip_runtime.h>

#include "../../include/iqgpu.h"
#include "dsp_device.hpp"
#include "iq_calib.hpp"
#include "kernels.hpp"

#ifndef IQGPU_NT_DC
#define IQGPU_NT_DC 1      // k_dc_prefix's streaming loop (both widths) reads the call's frames once, with the non-temporal hint (0.116 -> 0.105 ms on config 3)
#endif

namespace iqgpu {

__device__ __forceinline__ int lvl_hist(const FrontArgs &a, int i) { return (i < a.S) ? 4 * a.m[i] : kArbHist; }

// one half-band decimator stage over a level buffer: dst[j] = 0.5 x[2j+1-2m] + sum_q h[2q+1] x[2j-2q]
// (taps pre-scaled by 0.5).  M > 0: compile-time semi-length, two accumulator chains.
template <int M>
__device__ __forceinline__ void hb_stage(const cf2 *src, cf2 *dst, const float *taps, int n_out, int tid, int m_rt = 0)
{
    const int m = M > 0 ? M : m_rt;
    float h[M > 0 ? 2 * M : 1];
    if (M > 0) {
#pragma unroll
        for (int q = 0; q < 2 * M; ++q) h[q] = taps[q];
    }
    for (int jl = tid; jl < n_out; jl += kThreads) {
        const cf2 d = src[2 * jl + 1 - 2 * m];           // centre tap (delay branch), gain 0.5
        const cf2 *p = src + 2 * jl;
        float ar = 0.5f * d.x, ai = 0.5f * d.y;
        if (M > 0) {
            cf2 sv[M > 0 ? 2 * M : 1];
#pragma unroll
            for (int q = 0; q < 2 * M; ++q) sv[q] = p[-2 * q];
            float br = 0.0f, bi = 0.0f;
#pragma unroll
            for (int q = 0; q < 2 * M; q += 2) {             // same order within each chain as the rolled loop
                ar = fmaf(h[q], sv[q].x, ar); ai = fmaf(h[q], sv[q].y, ai);
                br = fmaf(h[q + 1], sv[q + 1].x, br); bi = fmaf(h[q + 1], sv[q + 1].y, bi);
            }
            ar += br; ai += bi;
        } else {
            for (int q = 0; q < 2 * m; ++q) {                // odd taps h[2q+1] on x[2jl - 2q]
                const cf2 sv = p[-2 * q];
                const float h = taps[q];
                ar = fmaf(h, sv.x, ar); ai = fmaf(h, sv.y, ai);
            }
        }
        dst[jl] = cf2{ar, ai};
    }
}

// ============================================================================================
// k_front
//   Block b owns tiles [b*tpb, (b+1)*tpb) of kTile input samples (tile boundaries are aligned to
//   the stream's 2^S groups) and first re-runs warm_tiles tiles to rebuild every stage window, so
//   blocks are independent; inside a block the tiles run in order and all state (dc blocker
//   value, stage histories, next output index) is carried in registers / LDS.
// ============================================================================================
__global__ __launch_bounds__(kThreads) void k_front(const FrontArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S;

    cf2   *s_nco = (cf2 *)smem;                              // 1024 {cos, sin}
    float *s_arb = (float *)(s_nco + 1024);                  // [256][16]
    float *s_hb  = s_arb + 256 * 16;                         // branch taps
    cf2   *s_wtot = (cf2 *)(s_hb + ((a.n_hb_taps + 3) & ~3)); // [2][4] dc wave totals
    cf2   *s_lvl = s_wtot + 8;                               // level buffers

    // ---- tables and zeroed histories ----
    if (a.nco_mode != 0 || a.pnco_mode != 0)
        for (int i = tid; i < 1024; i += kThreads) s_nco[i] = a.nco_tab[i];
    if (a.mode == 1) {
        for (int i = tid; i < 256 * 16; i += kThreads) s_arb[i] = a.arb_table[i];
        for (int i = tid; i < a.n_hb_taps; i += kThreads) s_hb[i] = a.hb_taps[i];
        const int total = a.lvl_off[S + 1];
        for (int i = tid; i < total; i += kThreads) s_lvl[i] = cf2{0.0f, 0.0f};
    }

    const int b = blockIdx.x;
    const int64_t t_emit0 = (int64_t)b * a.tiles_per_block;
    int64_t t_emit1 = t_emit0 + a.tiles_per_block;
    if (t_emit1 > a.total_tiles || b == (int)gridDim.x - 1) t_emit1 = a.total_tiles;
    const int64_t t_begin = t_emit0 - a.warm_tiles;
    const int TG = kTile >> S;
    const int bps = valid_frame_bytes(a.in_fmt);

    // ---- block 0 keeps the part of the old history that this (short) call does not replace ----
    if (b == 0 && a.frames_in < (int64_t)a.hist_cap) {
        const int keep = a.hist_cap - (int)a.frames_in;
        for (int i = tid; i < keep; i += kThreads) a.hist_out[i] = a.hist_in[i + (int)a.frames_in];
    }

    // ---- dc blocker state ----
    float vr = 0.0f, vi = 0.0f;       // v[n-1] at the start of the next chunk (uniform)
    bool dc_started = false;
    float lane_pow = 1.0f;            // c^(4*lane)
    if (a.dc_enable) {
#pragma unroll
        for (int k = 0; k < 6; ++k) if (lane & (1 << k)) lane_pow *= a.dc_cpow[k];
    }

    uint64_t k_next = 0;
    if (a.mode == 1) k_next = first_k_at((uint64_t)(t_emit0 * TG) << 24, a.phi0, a.step);

    __syncthreads();

    for (int64_t t = t_begin; t < t_emit1; ++t) {
        const int64_t i0 = t * kTile;             // group-aligned index of the tile's first sample
        const int64_t j0 = i0 - a.rem0;           // index into this call's new samples
        const bool emit = t >= t_emit0;
        const bool interior = (j0 >= 0) && (j0 + kTile <= a.frames_in) && a.raw_aligned &&
                              (((j0 * bps) & 15) == 0);
        cf2 *lv0 = s_lvl + a.lvl_off[0] + lvl_hist(a, 0);

        if (a.dc_enable && !dc_started && j0 + kTile > 0) {
            // state before the block's first new sample, moved back over the n_h history
            // positions of this tile that precede it (they feed zeros into the recurrence)
            const cd2 cv = a.dc_carry[b];
            const int64_t n_h = (j0 < 0) ? -j0 : 0;
            const double back = exp(-(double)n_h * a.dc_logc);
            vr = (float)(cv.x * back); vi = (float)(cv.y * back);
            dc_started = true;
        }

        // ------------------------------------------------------------ phase 1: pointwise
#pragma unroll
        for (int c = 0; c < kTile / 1024; ++c) {
            const int l = c * 1024 + 4 * tid;
            const int64_t j = j0 + l;
            cf2 x[4];
            bool is_hist[4] = {false, false, false, false};
            bool is_new[4] = {true, true, true, true};
            bool fast = false;
            if (interior) fast = unpack_four_fast(a.raw, j, a.in_fmt, a.gain, x);
            if (!fast) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int64_t js = j + s;
                    if (js < 0) {
                        const int64_t h = (int64_t)a.hist_cap + js;
                        x[s] = (h >= 0) ? a.hist_in[h] : cf2{0.0f, 0.0f};
                        is_hist[s] = true; is_new[s] = false;
                    } else if (js >= a.frames_in) {
                        x[s] = cf2{0.0f, 0.0f};
                        is_new[s] = false;
                    } else {
                        x[s] = unpack_one(a.raw, js, a.in_fmt, a.gain);
                    }
                }
            }

            if (a.dc_enable) {
                // v[n] = x[n] + c v[n-1];  y[n] = v[n] - v[n-1] = x[n] - (1-c) v[n-1]   (SPEC B.5)
                const float cc = a.dc_c;
                cf2 xd[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) xd[s] = is_hist[s] ? cf2{0.0f, 0.0f} : x[s];
                float br = xd[0].x, bi = xd[0].y;
#pragma unroll
                for (int s = 1; s < 4; ++s) { br = fmaf(br, cc, xd[s].x); bi = fmaf(bi, cc, xd[s].y); }
                // inclusive scan over the 64 lanes: B_l += c^(4*2^k) B_(l-2^k)
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const float ur = __shfl_up(br, 1 << k), ui = __shfl_up(bi, 1 << k);
                    if (lane >= (1 << k)) { br = fmaf(a.dc_cpow[k], ur, br); bi = fmaf(a.dc_cpow[k], ui, bi); }
                }
                cf2 *wt = s_wtot + 4 * (c & 1);
                if (lane == 63) wt[wave] = cf2{br, bi};
                float er = __shfl_up(br, 1), ei = __shfl_up(bi, 1);   // exclusive within the wave
                if (lane == 0) { er = 0.0f; ei = 0.0f; }
                __syncthreads();
                // state at this wave's first sample, and at the end of the chunk
                const float c256 = a.dc_cpow[6];
                float pr = vr, pi = vi;           // running state across the 4 waves
                float wr = 0.0f, wi = 0.0f;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    if (w == wave) { wr = pr; wi = pi; }
                    const cf2 tot = wt[w];
                    pr = fmaf(c256, pr, tot.x); pi = fmaf(c256, pi, tot.y);
                }
                vr = pr; vi = pi;
                float sr = fmaf(lane_pow, wr, er), si = fmaf(lane_pow, wi, ei);  // v[n-1] of x[0]
                const float aa = a.dc_a;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float yr = fmaf(-aa, sr, xd[s].x), yi = fmaf(-aa, si, xd[s].y);
                    sr = fmaf(cc, sr, xd[s].x); si = fmaf(cc, si, xd[s].y);
                    if (!is_hist[s]) { x[s].x = yr; x[s].y = yi; }
                }
            }

            if (a.iq_enable) { // src/iq_correct.c:307-313
#pragma unroll
                for (int s = 0; s < 4; ++s) if (!is_hist[s]) {
                    const float re = x[s].x;
                    x[s].x = re * a.iq_magp1;
                    x[s].y = fmaf(a.iq_phase, re, x[s].y);
                }
            }

            if (a.nco_mode != 0) {
                uint32_t th = a.nco_theta0 + (uint32_t)(i0 + l) * a.nco_dtheta;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if (!is_hist[s]) x[s] = nco_mix(x[s], nco_phasor(s_nco, th), a.nco_mode);
                    th += a.nco_dtheta;
                }
            }

            if (emit && a.hist_cap > 0 && j + 4 > a.frames_in - (int64_t)a.hist_cap) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int64_t back = a.frames_in - (j + s);      // 1 .. hist_cap for kept samples
                    if (is_new[s] && back <= (int64_t)a.hist_cap) a.hist_out[(int64_t)a.hist_cap - back] = x[s];
                }
            }

            if (a.mode == 1) {
                float4 *dst = (float4 *)(lv0 + l);
                dst[0] = make_float4(x[0].x, x[0].y, x[1].x, x[1].y);
                dst[1] = make_float4(x[2].x, x[2].y, x[3].x, x[3].y);
            } else if (emit) {
                // no resampler: frames map one to one (src/pipeline.c:516-519)
                uint32_t th = a.pnco_theta0 + (uint32_t)j * a.pnco_dtheta;
                cf2 yv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    cf2 y = x[s];
                    if (a.pnco_mode != 0) y = nco_mix(y, nco_phasor(s_nco, th), a.pnco_mode);
                    yv[s] = y;
                    th += a.pnco_dtheta;
                }
                pack_store_group<4>(a.out, j, a.out_fmt, yv, is_new);     // whole quads as one piece (dsp_device.hpp)
            }
        }
        if (a.mode != 1) continue;
        __syncthreads();

        // ------------------------------------------------------------ phase 2: half-band cascade
        for (int i = 0; i < S; ++i) {
            const int m = a.m[i], n_out = kTile >> (i + 1);
            const cf2 *src = s_lvl + a.lvl_off[i] + 4 * m;
            cf2 *dst = s_lvl + a.lvl_off[i + 1] + lvl_hist(a, i + 1);
            const float *taps = s_hb + a.tap_off[i];
            // liquid's designs at 60 dB use m = 10, 5, 3, 3, ...: those get fully unrolled bodies (all window
            // reads in flight at once); any other semi-length runs the rolled loop
            switch (m) {
            case 3:  hb_stage<3>(src, dst, a.hb_taps + a.tap_off[i], n_out, tid); break;    // uniform global reads:
            case 5:  hb_stage<5>(src, dst, a.hb_taps + a.tap_off[i], n_out, tid); break;    // s_load, taps in SGPRs
            case 10: hb_stage<10>(src, dst, a.hb_taps + a.tap_off[i], n_out, tid); break;
            default: hb_stage<0>(src, dst, taps, n_out, tid, m); break;
            }
            __syncthreads();
        }

        // ------------------------------------------------------------ phase 3: polyphase + pack
        if (emit) {
            const int64_t qa = t * TG;
            int64_t qb = qa + TG; if (qb > a.n_groups) qb = a.n_groups;
            if (qb > qa) {
                const uint64_t k_lo = k_next;
                uint64_t k_hi;
                if (qb - qa == TG) {
                    k_hi = k_lo + a.n_est;
                    while (a.phi0 + k_hi * (uint64_t)a.step < ((uint64_t)qb << 24)) ++k_hi;
                } else {
                    k_hi = first_k_at((uint64_t)qb << 24, a.phi0, a.step);
                }
                const cf2 *hb = s_lvl + a.lvl_off[S] + kArbHist;
                for (uint64_t k = k_lo + tid; k < k_hi; k += kThreads) {
                    const uint64_t P = a.phi0 + k * (uint64_t)a.step;
                    const int ql = (int)((int64_t)(P >> 24) - qa);
                    const int arm = (int)((P >> 16) & 255u);
                    const cf2 *w = hb + ql;
                    const float *tp = s_arb + arm * 16;
                    float ar = 0.0f, ai = 0.0f;
#pragma unroll
                    for (int n = 0; n < 14; ++n) {
                        const cf2 sv = w[-n];
                        ar = fmaf(tp[n], sv.x, ar); ai = fmaf(tp[n], sv.y, ai);
                    }
                    cf2 y{ar, ai};
                    if (a.pnco_mode != 0)
                        y = nco_mix(y, nco_phasor(s_nco, a.pnco_theta0 + (uint32_t)k * a.pnco_dtheta), a.pnco_mode);
                    pack_store(a.out, (int64_t)k, a.out_fmt, y);
                }
                k_next = k_hi;
            }
        }
        __syncthreads();

        // ------------------------------------------------------------ phase 4: slide histories
        for (int i = wave; i <= S; i += 4) {
            const int H = lvl_hist(a, i), n_i = kTile >> i;
            cf2 *buf = s_lvl + a.lvl_off[i];
            if (lane < H) { const cf2 v = buf[n_i + lane]; buf[lane] = v; }
        }
        __syncthreads();
    }
}

size_t front_lds_bytes(const FrontArgs &a)
{
    size_t bytes = 1024 * sizeof(cf2) + 256 * 16 * sizeof(float) + (size_t)((a.n_hb_taps + 3) & ~3) * sizeof(float) + 8 * sizeof(cf2);
    if (a.mode == 1) bytes += (size_t)a.lvl_off[a.S + 1] * sizeof(cf2);
    return bytes;
}

hipError_t launch_front(const FrontArgs &a, int n_blocks, hipStream_t s)
{
    const size_t lds = front_lds_bytes(a);
    static LdsAttrCache cache;
    if (lds > 64 * 1024) { const hipError_t e = cache.ensure((const void *)k_front, lds); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(k_front, dim3((unsigned)n_blocks), dim3(kThreads), lds, s, a);
    return hipGetLastError();
}

// ============================================================================================
// DC-blocker carries
// ============================================================================================
// a thread's four frames of one chunk (zeros where the chunk is padding) by Horner, folded into its accumulator: THE chunk arithmetic of
// dc_prefix_segment, whichever way the frames were loaded
__device__ __forceinline__ void dc_fold_chunk(float &accr, float &acci, const cf2 (&x)[4], float c, float c1024)
{
    float lr = 0.0f, li = 0.0f;
#pragma unroll
    for (int s = 0; s < 4; ++s) { lr = fmaf(lr, c, x[s].x); li = fmaf(li, c, x[s].y); }
    accr = fmaf(accr, c1024, lr); acci = fmaf(acci, c1024, li);
}

// whole rounds of NL chunks from chunk ch on, a thread's NL loads in flight at once; returns the first chunk not done.  The format is a
// compile-time argument and sets the width: FB bytes a frame, so a thread's four frames are one load of 4 FB bytes (16 for the 16-bit
// formats, 8 for the 8-bit ones) and NL = 16 / FB of them (4 / 8) are in flight.  base: the thread's four frames of chunk 0, aligned to a
// load.  One load at a time left the kernel at 4.4 TB/s on 16-bit frames (32 KiB in flight per CU) and at 1.2 TB/s on an RTL-SDR's cu8
// capture (late round 5: 0.42 ms per 2^28 frames, more than the resampler behind it).  Same arithmetic as the general chunk, same order.
template <int FMT>
__device__ __forceinline__ int64_t dc_stream_chunks(float &accr, float &acci, const char *base, int64_t ch, int64_t n_chunks, float gain, float c, float c1024)
{
    constexpr int FB = frame_bytes(FMT), NL = 16 / FB;
    static_assert(FB == 2 || FB == 4, "the 8-bit and 16-bit formats");
    typedef uint32_t wv __attribute__((ext_vector_type(FB)));      // four frames: FB words
    for (; ch + NL <= n_chunks; ch += NL) {
        wv v[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const wv *p = (const wv *)(base + (ch + i) * (1024 * FB));
#if IQGPU_NT_DC
            v[i] = __builtin_nontemporal_load(p);
#else
            v[i] = *p;
#endif
        }
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            cf2 x[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) x[s] = (FB == 4) ? unpack_b16(v[i][s], FMT, gain) : unpack_b8(v[i][s >> 1] >> (16 * (s & 1)), FMT, gain);
            dc_fold_chunk(accr, acci, x, c, c1024);
        }
    }
    return ch;
}

// One workgroup per segment: A = sum_k c^(end-1-k) x[k] over the segment's new samples.  ONE definition of a segment's aggregate:
// k_dc_prefix (a call) and k_dc_prefix_batch (the calls of a range, iqgpu_chain_*_dc_measure_range) both run it
__device__ __forceinline__ void dc_prefix_segment(const DcPrefixArgs &a, const int sgm)
{
    __shared__ float red[2 * 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t beg = dc_seg_start(a.geom, sgm);
    const int64_t end = (sgm == a.geom.n_seg - 1) ? a.geom.frames_in : dc_seg_start(a.geom, sgm + 1);
    const int64_t len = end - beg;
    float accr = 0.0f, acci = 0.0f;
    const int fb = frame_bytes(a.in_fmt);
    const bool vec_fmt = fb == 2 || fb == 4 || a.in_fmt == IQGPU_FMT_CF32;     // the formats of unpack_four_fast
    if (len > 0) {
        // left-pad the segment to whole chunks of 1024 so that the last chunk ends at `end`
        const int64_t n_chunks = (len + 1023) >> 10;
        const int64_t pad = (n_chunks << 10) - len;
        const float c = a.c;
        const float c1024 = (float)exp(1024.0 * a.logc);
        // chunk ch, any format and alignment; the first one holds the padding
        auto chunk = [&](int64_t ch) {
            const int64_t u = (ch << 10) + 4 * tid;       // padded position of this thread's 4 samples
            const int64_t k0 = beg + u - pad;
            cf2 x[4];
            // one coalesced vector load when the four frames are real and 16-byte aligned
            const bool vec = vec_fmt && a.raw_aligned && u >= pad && ((k0 * fb) & 15) == 0 && unpack_four_fast(a.raw, k0, a.in_fmt, a.gain, x);
            if (!vec) {
#pragma unroll
                for (int s = 0; s < 4; ++s) x[s] = (u + s >= pad) ? unpack_one(a.raw, k0 + s, a.in_fmt, a.gain) : cf2{0.0f, 0.0f};
            }
            dc_fold_chunk(accr, acci, x, c, c1024);
        };
        int64_t ch = 0;
        // 16-bit and 8-bit formats whose chunks start 16-byte aligned: the padded chunk, then whole rounds of four / eight chunks with
        // their loads in flight together (entered with more than 5 / 9 chunks: the padded one, a round, and a tail)
        if ((fb == 4 ? n_chunks > 5 : fb == 2 && n_chunks > 9) && a.raw_aligned && (((beg - pad) * fb) & 15) == 0) {
            chunk(0);
            const char *base = (const char *)a.raw + (beg - pad + 4 * tid) * fb;
            switch (a.in_fmt) {
            case IQGPU_FMT_CS16:    ch = dc_stream_chunks<IQGPU_FMT_CS16>(accr, acci, base, 1, n_chunks, a.gain, c, c1024); break;
            case IQGPU_FMT_CU16:    ch = dc_stream_chunks<IQGPU_FMT_CU16>(accr, acci, base, 1, n_chunks, a.gain, c, c1024); break;
            case IQGPU_FMT_SC16Q11: ch = dc_stream_chunks<IQGPU_FMT_SC16Q11>(accr, acci, base, 1, n_chunks, a.gain, c, c1024); break;
            case IQGPU_FMT_CU8:     ch = dc_stream_chunks<IQGPU_FMT_CU8>(accr, acci, base, 1, n_chunks, a.gain, c, c1024); break;
            default:                ch = dc_stream_chunks<IQGPU_FMT_CS8>(accr, acci, base, 1, n_chunks, a.gain, c, c1024); break;
            }
        }
        for (; ch < n_chunks; ++ch) chunk(ch);
        const float wt = (float)exp((double)(1020 - 4 * tid) * a.logc);  // to the end of the chunk
        accr *= wt; acci *= wt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { accr += __shfl_down(accr, o); acci += __shfl_down(acci, o); }
    if (lane == 0) { red[2 * wave] = accr; red[2 * wave + 1] = acci; }
    __syncthreads();
    if (tid == 0) {
        float r = 0.0f, i = 0.0f;
        for (int w = 0; w < 4; ++w) { r += red[2 * w]; i += red[2 * w + 1]; }
        a.agg[sgm] = cf2{r, i};
    }
}

// (7 waves per SIMD, the occupancy the kernel has run at: without the bound the scheduler converts all the frames of a round ahead of the
//  folds and takes 76 registers -- 6 waves; held to it, it converts as the loads arrive, in 45)
__global__ __launch_bounds__(kThreads, 7) void k_dc_prefix(const DcPrefixArgs a) { dc_prefix_segment(a, (int)blockIdx.x); }

// grid (segment, entry): entry blockIdx.y of the table is one piece of one call -- its geometry, where its frames start in raw, the
// alignment of that address, where its aggregates go -- and this workgroup does for segment blockIdx.x of it what k_dc_prefix does
__global__ __launch_bounds__(kThreads, 7) void k_dc_prefix_batch(const DcPrefixBatchArgs b)
{
    const DcBatchEntry e = b.entries[blockIdx.y];
    if ((int)blockIdx.x >= e.geom.n_seg) return;
    DcPrefixArgs a;
    a.raw = (const char *)b.raw + e.raw_off; a.in_fmt = b.in_fmt; a.gain = b.gain; a.raw_aligned = e.raw_aligned;
    a.c = b.c; a.logc = b.logc; a.geom = e.geom; a.agg = b.agg + e.agg_off;
    dc_prefix_segment(a, (int)blockIdx.x);
}

hipError_t launch_dc_prefix_batch(const DcPrefixBatchArgs &b, int n_entries, int max_seg, hipStream_t s)
{
    if (n_entries < 1 || n_entries > kDcBatchEntries || max_seg < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dc_prefix_batch, dim3((unsigned)max_seg, (unsigned)n_entries), dim3(kThreads), 0, s, b);
    return hipGetLastError();
}

hipError_t launch_dc_prefix(const DcPrefixArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_dc_prefix, dim3((unsigned)a.geom.n_seg), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

// the blocker's state behind a piece of stream whose map is v -> f v + g.  ONE definition: k_dc_scan's state update and k_dc_walk
// (iqgpu_chain_dc_advance) both call it, so a walked state is the ordinary path's bit for bit
__device__ inline cd2 dc_map_apply(double f, double gr, double gi, cd2 v) { return cd2{f * v.x + gr, f * v.y + gi}; }

constexpr int kDcScanThreads = 1024;      // one workgroup, 3 segments a thread for a launch of 3 072 runs: 11.7 us (256 threads: 17.8 us; loading the
                                          // aggregates ahead of the folds changes nothing -- the folds' 64-bit index arithmetic and the barriers of the scan do)
// carry[s] = state before segment s; state <- state after the last sample.  The per-segment maps
// v -> f_s v + g_s (f_s = c^len_s, g_s = the segment's aggregate) compose associatively: each of the
// threads folds a contiguous slice of segments, the slices are scanned through LDS, then every thread
// replays its slice from its prefix.  All in double.
// ONE definition of the fold and the scan: k_dc_scan (a call) and k_dc_scan_batch (the calls of a range) both run it.  Behind it
// sf / sr / si[tid] hold the inclusive scan of the slices' maps; [kDcScanThreads - 1]: the map of the whole call
struct DcScanSlice { int s0, s1; };
__device__ __forceinline__ int64_t dc_seg_len(const DcGeom &g, int sgm)
{
    const int64_t beg = dc_seg_start(g, sgm);
    const int64_t end = (sgm == g.n_seg - 1) ? g.frames_in : dc_seg_start(g, sgm + 1);
    return end > beg ? end - beg : (int64_t)0;
}
__device__ __forceinline__ DcScanSlice dc_scan_fold(const DcGeom &geom, const cf2 *agg, const double logc, double *sf, double *sr, double *si)
{
    const int tid = threadIdx.x;
    const int n = geom.n_seg;
    const int per = (n + kDcScanThreads - 1) / kDcScanThreads;
    const int s0 = tid * per, s1 = (s0 + per < n) ? s0 + per : n;
    // fold the slice: v_out = F v_in + (Gr, Gi)
    double F = 1.0, Gr = 0.0, Gi = 0.0;
    {
        int64_t prev_len = -1; double f = 1.0;
        for (int sgm = s0; sgm < s1; ++sgm) {
            const int64_t len = dc_seg_len(geom, sgm);
            if (len != prev_len) { f = exp((double)len * logc); prev_len = len; }
            const cf2 g = agg[sgm];
            F *= f; Gr = Gr * f + (double)g.x; Gi = Gi * f + (double)g.y;
        }
    }
    sf[tid] = F; sr[tid] = Gr; si[tid] = Gi;
    __syncthreads();
    // inclusive scan of the maps (later map applied after the earlier one)
    for (int o = 1; o < kDcScanThreads; o <<= 1) {
        double pf = 1.0, pr = 0.0, pi = 0.0;
        const bool has = tid >= o;
        if (has) { pf = sf[tid - o]; pr = sr[tid - o]; pi = si[tid - o]; }
        __syncthreads();
        if (has) { sr[tid] = sr[tid] + sf[tid] * pr; si[tid] = si[tid] + sf[tid] * pi; sf[tid] = sf[tid] * pf; }
        __syncthreads();
    }
    return DcScanSlice{s0, s1};
}
// the measure pass: the call's whole map and nothing else, map[0] = {F, 0}, map[1] = G
__device__ __forceinline__ void dc_scan_store_map(cd2 *map, const double *sf, const double *sr, const double *si)
{
    const int tid = threadIdx.x;
    if (tid == kDcScanThreads - 1) { map[0] = cd2{sf[tid], 0.0}; map[1] = cd2{sr[tid], si[tid]}; }
}

__global__ __launch_bounds__(kDcScanThreads) void k_dc_scan(const DcScanArgs a)
{
    __shared__ double sf[kDcScanThreads], sr[kDcScanThreads], si[kDcScanThreads];
    const int tid = threadIdx.x;
    const DcScanSlice sl = dc_scan_fold(a.geom, a.agg, a.logc, sf, sr, si);
    const int s0 = sl.s0, s1 = sl.s1;
    // the measure pass (iqgpu_chain_dc_measure): state and carries stay as they are
    if (a.map) { dc_scan_store_map(a.map, sf, sr, si); return; }
    const double v0r = a.state->x, v0i = a.state->y;
    // state before this thread's slice = (inclusive scan of the previous thread) applied to v0
    double vr = v0r, vi = v0i;
    if (tid > 0) { vr = sf[tid - 1] * v0r + sr[tid - 1]; vi = sf[tid - 1] * v0i + si[tid - 1]; }
    {
        int64_t prev_len = -1; double f = 1.0;
        for (int sgm = s0; sgm < s1; ++sgm) {
            a.carry[sgm] = cd2{vr, vi};
            const int64_t len = dc_seg_len(a.geom, sgm);
            if (len != prev_len) { f = exp((double)len * a.logc); prev_len = len; }
            const cf2 g = a.agg[sgm];
            vr = vr * f + (double)g.x; vi = vi * f + (double)g.y;
        }
    }
    __syncthreads();
    if (tid == kDcScanThreads - 1) *a.state = dc_map_apply(sf[tid], sr[tid], si[tid], cd2{v0r, v0i});
}

// one workgroup per entry of the table: the map-only branch of k_dc_scan for that piece, into map[2 entry], map[2 entry + 1]
__global__ __launch_bounds__(kDcScanThreads) void k_dc_scan_batch(const DcScanBatchArgs b)
{
    __shared__ double sf[kDcScanThreads], sr[kDcScanThreads], si[kDcScanThreads];
    const DcBatchEntry e = b.entries[blockIdx.x];
    dc_scan_fold(e.geom, b.agg + e.agg_off, b.logc, sf, sr, si);
    dc_scan_store_map(b.map + 2 * (size_t)blockIdx.x, sf, sr, si);
}

hipError_t launch_dc_scan_batch(const DcScanBatchArgs &b, int n_entries, hipStream_t s)
{
    if (n_entries < 1 || n_entries > kDcBatchEntries) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dc_scan_batch, dim3((unsigned)n_entries), dim3(kDcScanThreads), 0, s, b);
    return hipGetLastError();
}

hipError_t launch_dc_scan(const DcScanArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_dc_scan, dim3(1), dim3(kDcScanThreads), 0, s, a);
    return hipGetLastError();
}

// iqgpu_chain_dc_advance: *state walked over n per-call maps in order, before[k] = the state in front of map k.  One thread: the
// walk is a chain of n dependent multiply-adds.
__global__ __launch_bounds__(64) void k_dc_walk(const DcWalkArgs a)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    cd2 v = *a.state;
    for (int64_t k = 0; k < a.n; ++k) {
        if (a.before) a.before[k] = v;
        const DcMapRow r = a.rows[k];
        v = dc_map_apply(r.f, r.g_re, r.g_im, v);
    }
    *a.state = v;
}

hipError_t launch_dc_walk(const DcWalkArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_dc_walk, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

// ============================================================================================
// k_fir: y[i] = sum_k h[k] f[(L-1) + i - k]   (firfilt / fftfilt are the same linear convolution,
// SPEC B.2/B.3); taps and the matching data window are staged through LDS in chunks of
// kFirTapChunk taps; each thread owns four outputs 256 apart so LDS reads are conflict free.
// ============================================================================================
__global__ __launch_bounds__(kThreads) void k_fir(const FirArgs a)
{
    __shared__ __align__(16) cf2 s_w[kFirOutTile + kFirTapChunk];
    __shared__ __align__(16) cf2 s_h[kFirTapChunk];
    __shared__ __align__(16) cf2 s_nco[1024];
    const int tid = threadIdx.x;
    const int64_t o0 = (int64_t)blockIdx.x * kFirOutTile;
    const int L = a.ntaps;
    if (a.pnco_mode != 0) for (int i = tid; i < 1024; i += kThreads) s_nco[i] = a.nco_tab[i];
    if (a.move_n > 0 && blockIdx.x == gridDim.x - 1)
        for (int64_t i = tid; i < a.move_n; i += kThreads) a.move_dst[i] = a.move_src[i];

    float ar[4] = {0, 0, 0, 0}, ai[4] = {0, 0, 0, 0};
    for (int k0 = 0; k0 < L; k0 += kFirTapChunk) {
        __syncthreads();
        // window element e <-> f index base + e, base = (L-1) + o0 - k0 - (C-1)
        const int64_t base = (int64_t)(L - 1) + o0 - k0 - (kFirTapChunk - 1);
        const int64_t fmax = (int64_t)(L - 1) + a.n_emit;   // valid f indices are [0, fmax)
        for (int e = tid; e < kFirOutTile + kFirTapChunk - 1; e += kThreads) {
            const int64_t fi = base + e;
            s_w[e] = (fi >= 0 && fi < fmax) ? a.fbuf[fi] : cf2{0.0f, 0.0f};
        }
        for (int e = tid; e < kFirTapChunk; e += kThreads)
            s_h[e] = (k0 + e < L) ? a.taps[k0 + e] : cf2{0.0f, 0.0f};
        __syncthreads();
        const int kn = (L - k0 < kFirTapChunk) ? L - k0 : kFirTapChunk;
        if (a.is_complex) {
            for (int kk = 0; kk < kn; ++kk) {
                const cf2 h = s_h[kk];
                const cf2 *p = s_w + tid + (kFirTapChunk - 1) - kk;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const cf2 x = p[256 * r];
                    ar[r] = fmaf(h.x, x.x, ar[r]); ar[r] = fmaf(-h.y, x.y, ar[r]);
                    ai[r] = fmaf(h.x, x.y, ai[r]); ai[r] = fmaf(h.y, x.x, ai[r]);
                }
            }
        } else {
            for (int kk = 0; kk < kn; ++kk) {
                const float h = s_h[kk].x;
                const cf2 *p = s_w + tid + (kFirTapChunk - 1) - kk;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const cf2 x = p[256 * r];
                    ar[r] = fmaf(h, x.x, ar[r]); ai[r] = fmaf(h, x.y, ai[r]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = o0 + tid + 256 * r;
        if (i < a.n_emit) {
            cf2 y{ar[r], ai[r]};
            if (a.pnco_mode != 0)
                y = nco_mix(y, nco_phasor(s_nco, a.pnco_theta0 + (uint32_t)i * a.pnco_dtheta), a.pnco_mode);
            pack_store(a.out, i, a.out_fmt, y);
        }
    }
}

hipError_t launch_fir(const FirArgs &a, hipStream_t s)
{
    if (a.n_emit <= 0) return hipSuccess;
    const unsigned nb = (unsigned)((a.n_emit + kFirOutTile - 1) / kFirOutTile);
    hipLaunchKernelGGL(k_fir, dim3(nb), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

__global__ void k_copy_cf(cf2 *dst, const cf2 *src, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

hipError_t launch_copy_cf(cf2 *dst, const cf2 *src, int64_t n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    unsigned nb = (unsigned)((n + 255) / 256); if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(k_copy_cf, dim3(nb), dim3(256), 0, s, dst, src, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// k_iq_probe: the block the reference hands to its I/Q optimiser -- the first 1024 samples of a chunk after
// unpack -> [dc block] -> [iq correct] -> [pre NCO]  (src/pipeline.c:468-476 copies them out of buffer A right
// behind pre_processor_apply_chain).  One wavefront; the dc recurrence (1024 steps) runs on one lane.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_iq_probe(const IqProbeArgs a)
{
    __shared__ cf2 x[1024];
    const int lane = threadIdx.x;
    float vr = 0.0f, vi = 0.0f;
    if (a.dc_enable && lane == 0) {
        const cd2 st = *a.dc_state;                // v[n-1] in front of this call's first sample
        vr = (float)st.x; vi = (float)st.y;
    }
    iq_block_head(x, a.raw, 0, a.in_fmt, a.gain, a.dc_enable != 0, a.dc_c, vr, vi, lane);     // (shared with k_iq_blocks, iq_calib.hpp)
    for (int i = lane; i < 1024; i += 64) {
        cf2 v = x[i];
        if (a.iq_enable) { const float re = v.x; v.x = re * a.iq_magp1; v.y = fmaf(a.iq_phase, re, v.y); }
        if (a.nco_mode != 0) v = nco_mix(v, nco_phasor(a.nco_tab, a.nco_theta0 + (uint32_t)i * a.nco_dtheta), a.nco_mode);
        a.out[i] = v;
    }
}

hipError_t launch_iq_probe(const IqProbeArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_iq_probe, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

} // namespace iqgpu
