// Tetra-mode channeliser: oversampled uniform-DFT polyphase filter bank (definition:
// oracle/pfb_np.py; the reference has no channeliser).
//   y_k[m] = sum_l h[l] x[mD - l] exp(-2 pi i k (mD - l) / M)
//          = sum_{r'} u_m[r'] exp(+2 pi i k r' / M),   u_m[r'] = v_m[(r' + mD) mod M],
//   v_m[r] = sum_p h[r + pM] x[mD - r - pM]                       (P taps per branch)
// One workgroup produces T consecutive output times of all M channels:
//   stage 0  coalesced load + format conversion of (T-1)D + MP input samples into LDS
//   stage A  polyphase branch sums v, written circularly shifted (u)
//   stage B  M-point DFT as M1 x M2 Cooley-Tukey
// Output layout [M][n_out] cf32 (channel-major), which is the [carriers][n] input of TETRA mode.
// Two kernels: k_pfb_fft (register-resident mixed-radix small DFTs, any D whose input window fits
// LDS) and k_pfb (direct small DFTs, T chosen to fit) as the general fallback.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chan_stream.hpp"
#include "small_dft.hpp"
#include "wire_format.hpp"

namespace tdm {

constexpr int kPfbThreads = 256;

struct PfbParams {
    int32_t D;        // decimation
    int32_t T;        // output times per workgroup
    int32_t fmt;      // TDM_CU8 / TDM_CS8 / TDM_CF32 / TDM_CS16
    int32_t pad_;
    int64_t n_in, n_out;
    const float *h;       // [M*P] prototype
    const float2 *W1;     // [M1][M1]  exp(+2 pi i k1 n1 / M1)
    const float2 *WM;     // [M1][M2]  exp(+2 pi i k1 n2 / M)
    const float2 *W2;     // [M2][M2]  exp(+2 pi i k2 n2 / M2)
    int32_t G;            // k_pfb_fft: rounds of TB output times per workgroup
    int32_t pad2_;
    int64_t in_stride;    // bytes between the input streams of a batch (grid.y)
    int64_t out_batch;    // float2 elements between the outputs of a batch
    // carried state of a stream (tdm_channeliser, chan_stream.hpp); a stateless call has hist = nullptr and zeros here.
    // Local input n < 0 reads history slot n + (L-1) when n >= -hist_valid, else zero; output m's window ends at local
    // input o + m*D, its phase shift is (s_base + m*D) mod M.
    const void *hist;     // [grid.y] streams of L-1 samples in wire format, hist_stride bytes apart
    int64_t hist_stride;
    int64_t hist_valid;
    int64_t o;
    int32_t s_base;
    int32_t pad3_;
};

// one past the last history sample of stream y (local index n < 0 lives at byte n * fb from here, fb = the format's bytes per
// sample), or nullptr
template <int L>
__device__ __forceinline__ const char *pfb_hist_end(const PfbParams &Q, int y, int fb)
{
    return Q.hist ? (const char *)Q.hist + (int64_t)y * Q.hist_stride + (int64_t)(L - 1) * fb : nullptr;
}


__device__ __forceinline__ float2 pfb_load(const void *iq, int fmt, int64_t n)
{
    if (fmt == FMT_CU8) {
        const uint8_t *p = (const uint8_t *)iq + 2 * n;
        return make_float2(wire_f32<FMT_CU8>(p[0]), wire_f32<FMT_CU8>(p[1]));
    } else if (fmt == FMT_CS8) {
        const int8_t *p = (const int8_t *)iq + 2 * n;
        return make_float2(wire_f32<FMT_CS8>(p[0]), wire_f32<FMT_CS8>(p[1]));
    } else if (fmt == FMT_CS16) {
        const int16_t *p = (const int16_t *)iq + 2 * n;
        return make_float2(wire_f32<FMT_CS16>(p[0]), wire_f32<FMT_CS16>(p[1]));
    }
    return ((const float2 *)iq)[n];
}

__device__ __forceinline__ float2 cfma(float2 a, float2 b, float2 acc)
{
    acc.x = fmaf(a.x, b.x, acc.x);
    acc.x = fmaf(-a.y, b.y, acc.x);
    acc.y = fmaf(a.x, b.y, acc.y);
    acc.y = fmaf(a.y, b.x, acc.y);
    return acc;
}

template <int M1, int M2, int P>
__global__ __launch_bounds__(kPfbThreads) void k_pfb(const void *__restrict__ iq, float2 *__restrict__ out,
                                                      int64_t out_stride, const PfbParams Q)
{
    constexpr int M = M1 * M2;
    constexpr int L = M * P;
    constexpr int RS = M + 1;  // padded row stride of u / A
    extern __shared__ float2 smem[];
    const int T = Q.T, D = Q.D;
    const int nxs = (T - 1) * D + L;
    float2 *xs = smem;                 // [nxs]
    float2 *u = xs + nxs;              // [T][RS]
    float2 *A = u + T * RS;            // [T][RS]
    float2 *w1 = A + T * RS;           // [M1*M1]
    float2 *wm = w1 + M1 * M1;         // [M]
    float2 *w2 = wm + M;               // [M2*M2]
    const int tid = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * T;
    iq = (const char *)iq + (int64_t)blockIdx.y * Q.in_stride;
    out += (int64_t)blockIdx.y * Q.out_batch;
    const char *hend = pfb_hist_end<L>(Q, blockIdx.y, wire_bytes_fp32(Q.fmt));
    // ---- stage 0: inputs n = o + m0*D - (L-1) + i; n < 0 from the history (one load expression for both sources)
    const int64_t nbase = Q.o + m0 * D - (L - 1);
    for (int i = tid; i < nxs; i += kPfbThreads) {
        const int64_t n = nbase + i;
        const bool have = n >= 0 ? n < Q.n_in : n >= -Q.hist_valid;
        xs[i] = have ? pfb_load(n >= 0 ? iq : (const void *)hend, Q.fmt, n) : make_float2(0.f, 0.f);
    }
    for (int i = tid; i < M1 * M1; i += kPfbThreads) w1[i] = Q.W1[i];
    for (int i = tid; i < M; i += kPfbThreads) wm[i] = Q.WM[i];
    for (int i = tid; i < M2 * M2; i += kPfbThreads) w2[i] = Q.W2[i];
    __syncthreads();
    // ---- stage A: branch sums, stored circularly shifted by s = (m*D) mod M
    for (int idx = tid; idx < T * M; idx += kPfbThreads) {
        const int mi = idx / M, r = idx - mi * M;
        float2 acc = make_float2(0.f, 0.f);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const float hv = Q.h[r + p * M];
            const float2 xv = xs[mi * D + (L - 1) - r - p * M];
            acc.x = fmaf(hv, xv.x, acc.x);
            acc.y = fmaf(hv, xv.y, acc.y);
        }
        const int s = (int)((Q.s_base + ((m0 + mi) * (int64_t)D) % M) % M);
        int rp = r - s;
        if (rp < 0) rp += M;
        u[mi * RS + rp] = acc;
    }
    __syncthreads();
    // ---- stage B1: for each (mi, n2): M1-point DFT over n1, times the middle twiddle
    for (int idx = tid; idx < T * M2; idx += kPfbThreads) {
        const int mi = idx / M2, n2 = idx - mi * M2;
        float2 x[M1];
#pragma unroll
        for (int n1 = 0; n1 < M1; ++n1) x[n1] = u[mi * RS + M2 * n1 + n2];
#pragma unroll
        for (int k1 = 0; k1 < M1; ++k1) {
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int n1 = 0; n1 < M1; ++n1) acc = cfma(x[n1], w1[k1 * M1 + n1], acc);
            const float2 tw = wm[k1 * M2 + n2];
            A[mi * RS + k1 * M2 + n2] = make_float2(acc.x * tw.x - acc.y * tw.y, acc.x * tw.y + acc.y * tw.x);
        }
    }
    __syncthreads();
    // ---- stage B2: for each (k1, mi): M2-point DFT over n2 -> channels k = k1 + M1*k2
    for (int idx = tid; idx < T * M1; idx += kPfbThreads) {
        const int k1 = idx / T, mi = idx - k1 * T;
        float2 a[M2];
#pragma unroll
        for (int n2 = 0; n2 < M2; ++n2) a[n2] = A[mi * RS + k1 * M2 + n2];
        const int64_t m = m0 + mi;
#pragma unroll 4
        for (int k2 = 0; k2 < M2; ++k2) {
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int n2 = 0; n2 < M2; ++n2) acc = cfma(a[n2], w2[k2 * M2 + n2], acc);
            if (m < Q.n_out) out[(int64_t)(k1 + M1 * k2) * out_stride + m] = acc;
        }
    }
}

// ---- register-FFT variant ---------------------------------------------------------------------
// Workgroup = TB*M2 threads, TB consecutive output times per round, G rounds, any decimation D.
//   load     the round's input window arrives as 4-sample units prefetched into registers during
//            the previous round (one 8-byte load per unit for cu8/cs8, one 16-byte load for cs16, two for cf32),
//            converted and written to LDS with 16-byte stores
//   stage A  item = (branch r, group of 4 output times): the P taps of the branch stay in registers,
//            lanes walk consecutive r (conflict-free LDS reads and writes); the circular shift
//            (m*D) mod M of each output time is applied to the write index
//   pass 1   thread (mi, n2): SmallDft<M1> over n1 in place in the exchange tile, times the middle twiddle
//   pass 2   thread (k1, mi): SmallDft<M2> over n2, stores channels k1 + M1*k2; consecutive lanes hold
//            consecutive output times, so each channel row receives TB*8 contiguous bytes.
// wire_format.hpp's fp32 decode of a packed sample on the kernel's vector type (both components in one packed operation)
template <int FMT>
__device__ __forceinline__ cf32v pfb_decode(uint32_t w)
{
    const cf32v c = cv((float)wire_code_i<FMT>(w), (float)wire_code_q<FMT>(w)) * WireScale<FMT>::f32;
    return WireScale<FMT>::biased ? c - cv(1.f, 1.f) : c;
}
template <int FMT>
struct PfbUnit;   // four consecutive input samples in wire format + validity
template <>
struct PfbUnit<FMT_CF32> {
    float4 a, b;
    uint32_t ok;
    __device__ __forceinline__ void load(const char *base, const char *hend, int64_t hv, int64_t n0, int64_t n_in)
    {
        ok = 0;
        a = b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n0 >= 0 && n0 + 3 < n_in) {
            const float4 *p = (const float4 *)(base + n0 * 8);   // cf32 streams are 8-byte aligned
            __builtin_memcpy(&a, p, 16);
            __builtin_memcpy(&b, p + 1, 16);
            ok = 15u;
        } else {
            // per sample: the push (n >= 0) or the history (-hv <= n < 0), else zero
            float2 t[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t n = n0 + c;
                t[c] = make_float2(0.f, 0.f);
                if (n >= 0 ? n < n_in : n >= -hv) t[c] = ((const float2 *)(n >= 0 ? base : hend))[n];
            }
            const float2 t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
            a = make_float4(t0.x, t0.y, t1.x, t1.y);
            b = make_float4(t2.x, t2.y, t3.x, t3.y);
            ok = 15u;   // zeros already in place
        }
    }
    __device__ __forceinline__ void store(cf32v *dst) const
    {
        ((float4 *)dst)[0] = a;
        ((float4 *)dst)[1] = b;
    }
};
template <>
struct PfbUnit<FMT_CS16> {   // cs16: 16 bytes at a 4-byte aligned address; a word is int16 I (low half), int16 Q
    uint4 v;
    uint32_t ok;
    __device__ __forceinline__ void load(const char *base, const char *hend, int64_t hv, int64_t n0, int64_t n_in)
    {
        v = make_uint4(0u, 0u, 0u, 0u);
        if (n0 >= 0 && n0 + 3 < n_in) {
            __builtin_memcpy(&v, base + n0 * 4, 16);
            ok = 15u;
        } else {
            ok = 0;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t n = n0 + c;   // the push (n >= 0) or the history (-hv <= n < 0), in wire format either way
                if (n >= 0 ? n < n_in : n >= -hv) {
                    w[c] = ((const uint32_t *)(n >= 0 ? base : hend))[n];
                    ok |= 1u << c;
                }
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    __device__ __forceinline__ static cf32v conv(uint32_t w)
    {
        return pfb_decode<FMT_CS16>(w);
    }
    __device__ __forceinline__ void store(cf32v *dst) const
    {
        // (a sample that is not there was loaded as zero bits, which convert to 0.0: no mask needed)
        const cf32v s0 = conv(v.x), s1 = conv(v.y), s2 = conv(v.z), s3 = conv(v.w);
        float4 lo, hi;
        lo.x = s0.x; lo.y = s0.y; lo.z = s1.x; lo.w = s1.y;
        hi.x = s2.x; hi.y = s2.y; hi.z = s3.x; hi.w = s3.y;
        ((float4 *)dst)[0] = lo;
        ((float4 *)dst)[1] = hi;
    }
};
template <int FMT>
struct PfbUnit {   // FMT_CU8 / FMT_CS8: 8 bytes
    uint2 v;
    uint32_t ok;
    __device__ __forceinline__ void load(const char *base, const char *hend, int64_t hv, int64_t n0, int64_t n_in)
    {
        v = make_uint2(0u, 0u);
        if (n0 >= 0 && n0 + 3 < n_in) {
            __builtin_memcpy(&v, base + n0 * 2, 8);
            ok = 15u;
        } else {
            ok = 0;
            uint32_t w0 = 0u, w1 = 0u;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t n = n0 + c;   // the push (n >= 0) or the history (-hv <= n < 0), in wire format either way
                if (n >= 0 ? n < n_in : n >= -hv) {
                    const uint32_t h = ((const uint16_t *)(n >= 0 ? base : hend))[n];
                    if (c < 2) w0 |= h << (16 * (c & 1));
                    else w1 |= h << (16 * (c & 1));
                    ok |= 1u << c;
                }
            }
            v = make_uint2(w0, w1);
        }
    }
    __device__ __forceinline__ static cf32v conv(uint32_t h)   // low 16 bits: I, Q
    {
        return pfb_decode<FMT>(h);
    }
    __device__ __forceinline__ void store(cf32v *dst) const
    {
        cf32v s0 = conv(v.x), s1 = conv(v.x >> 16), s2 = conv(v.y), s3 = conv(v.y >> 16);
        if (ok != 15u) {
            if (!(ok & 1u)) s0 = cv(0.f, 0.f);
            if (!(ok & 2u)) s1 = cv(0.f, 0.f);
            if (!(ok & 4u)) s2 = cv(0.f, 0.f);
            if (!(ok & 8u)) s3 = cv(0.f, 0.f);
        }
        float4 lo, hi;
        lo.x = s0.x; lo.y = s0.y; lo.z = s1.x; lo.w = s1.y;
        hi.x = s2.x; hi.y = s2.y; hi.z = s3.x; hi.w = s3.y;
        ((float4 *)dst)[0] = lo;
        ((float4 *)dst)[1] = hi;
    }
};

// waves per SIMD that let `wgs` workgroups of nt threads share a CU
constexpr int pfb_waves_per_simd(int nt, int wgs) { return (wgs * ((nt + 63) / 64) + 3) / 4; }

template <int M1, int M2>
struct PfbFftGeom {
    static constexpr int FS = (M1 * M2) | 1;      // odd stride between output times of the exchange tile
};
// LDS footprint in float2 elements: input window + exchange tile + middle twiddles
template <int M1, int M2, int P, int TB>
constexpr size_t pfb_fft_lds(int D)
{
    const size_t xs = ((size_t)(TB - 1) * D + (size_t)M1 * M2 * P + 3) / 4 * 4;
    return xs + (size_t)TB * PfbFftGeom<M1, M2>::FS + (size_t)M1 * M2;
}

// ---- the three compute phases of a round (TB output times), shared by the kernel variants ----
// stage A: item = tid + it*NT -> (group of 4 output times, branch r).  All LDS reads of an item come
// before its writes (window and tile live in the same LDS array, so the compiler keeps their order);
// the opaque copy of tid keeps the per-item address arithmetic inside the round instead of hoisted
// into spilled registers.
template <int M1, int M2, int P, int TB>
__device__ __forceinline__ void pfb_stage_a(const cf32v *xs, cf32v *A, const float (*hv)[P], int tid, int D, int dmod, int s0)
{
    constexpr int M = M1 * M2, L = M * P, NT = TB * M2, FS = PfbFftGeom<M1, M2>::FS, FG = 4, NI = M1 / 4;
    int tid_v = tid;
    asm volatile("" : "+v"(tid_v));
#pragma unroll
    for (int it = 0; it < NI; ++it) {
        const int item = tid_v + it * NT;
        const int f = (item / M) * FG, r = item - (item / M) * M;
        const cf32v *px = xs + f * D + (L - 1) - r;
        cf32v acc[FG];
#pragma unroll
        for (int j = 0; j < FG; ++j) {
            acc[j] = px[j * D] * hv[it][0];
#pragma unroll
            for (int p = 1; p < P; ++p) acc[j] += px[j * D - p * M] * hv[it][p];
        }
        int sft = (int)(((uint32_t)s0 + (uint32_t)f * (uint32_t)dmod) % (uint32_t)M);
        cf32v *pa = A + f * FS;
#pragma unroll
        for (int j = 0; j < FG; ++j) {
            int rp = r - sft;   // branch r lands at (r - shift) mod M of output time f + j
            rp += rp < 0 ? M : 0;
            pa[j * FS + rp] = acc[j];
            sft += dmod;
            sft -= sft >= M ? M : 0;
        }
    }
}
// pass 1, in place: thread (mi, n2) owns column n2 of its output time
template <int M1, int M2>
__device__ __forceinline__ void pfb_pass1(cf32v *A, const cf32v *wml, int mi, int n2)
{
    cf32v x[M1];
    cf32v *col = A + mi * PfbFftGeom<M1, M2>::FS + n2;
#pragma unroll
    for (int n1 = 0; n1 < M1; ++n1) x[n1] = col[n1 * M2];
    SmallDft<M1>::run(x);
#pragma unroll
    for (int k1 = 0; k1 < M1; ++k1) col[k1 * M2] = cmulv(x[k1], wml[k1 * M2 + n2]);
}
// pass 2: thread (k1b, mib) transforms row k1b of output time mib and stores channels k1b + M1*k2
template <int M1, int M2>
__device__ __forceinline__ void pfb_pass2(const cf32v *A, cf32v *out, int64_t out_stride, int64_t m0, int64_t n_out,
                                          int k1b, int mib)
{
    cf32v a[M2];
    const cf32v *row = A + mib * PfbFftGeom<M1, M2>::FS + k1b * M2;
#pragma unroll
    for (int j = 0; j < M2; ++j) a[j] = row[j];
    SmallDft<M2>::run(a);
    const int64_t m = m0 + mib;
    if (m < n_out) {
        cf32v *po = out + (int64_t)k1b * out_stride + m;
        const int64_t step = (int64_t)M1 * out_stride;
#pragma unroll
        for (int k2 = 0; k2 < M2; ++k2) {
            __builtin_nontemporal_store(a[k2], po);
            po += step;
        }
    }
}

// NPF: 4-sample units per thread held in registers for the next round; WGS: workgroups per CU aimed at;
// CARRY: reads the carried state of Q (tdm_channeliser).  The stateless instantiation compiles the state away.
template <int M1, int M2, int P, int TB, int FMT, int NPF, int WGS, bool CARRY>
__global__ __launch_bounds__(TB *M2, pfb_waves_per_simd(TB *M2, WGS)) void k_pfb_fft(
    const void *__restrict__ iq_, cf32v *__restrict__ out_, int64_t out_stride, const PfbParams Q)
{
    static_assert(M1 <= M2, "pass 2 uses the first TB*M1 threads");
    static_assert(TB % 4 == 0 && M1 % 4 == 0, "stage A: M1/4 items of four output times per thread");
    constexpr int M = M1 * M2, L = M * P, NT = TB * M2;
    constexpr int NI = M1 / 4;   // M*(TB/4) items over NT threads
    extern __shared__ cf32v smem_v[];
    const int D = Q.D;
    const int nxs = (TB - 1) * D + L;
    const int nu = (nxs + 3) >> 2;
    const int dmod = D % M;
    cf32v *xs = smem_v;              // [4*nu]
    cf32v *A = smem_v + 4 * nu;      // [TB][FS]: row k1 (or n1) of an output time at k1*M2
    cf32v *wml = smem_v + (pfb_fft_lds<M1, M2, P, TB>(D) - M);   // [M1][M2] middle twiddles
    // (in LDS rather than re-read from memory: loads and stores share vmcnt, so a global load issued after
    //  pass 2's stores would wait for their write acknowledgements)
    const char *iq = (const char *)iq_ + (int64_t)blockIdx.y * Q.in_stride;
    const char *hend = CARRY ? pfb_hist_end<L>(Q, blockIdx.y, wire_bytes(FMT)) : nullptr;
    const int64_t hv = CARRY ? Q.hist_valid : 0, o = CARRY ? Q.o : 0;
    cf32v *out = out_ + (int64_t)blockIdx.y * Q.out_batch;
    const int tid = threadIdx.x;
    const int mi = tid / M2, n2 = tid - mi * M2;
    const int k1b = tid / TB, mib = tid - k1b * TB;
    float hv_taps[NI][P];   // taps of this thread's stage-A branches (the same in every round)
#pragma unroll
    for (int it = 0; it < NI; ++it) {
        const int item = tid + it * NT;
        const int r = item - (item / M) * M;
#pragma unroll
        for (int p = 0; p < P; ++p) hv_taps[it][p] = Q.h[r + p * M];
    }
    for (int i = tid; i < M; i += NT) {
        const float2 w = Q.WM[i];
        wml[i] = cv(w.x, w.y);
    }
    const int64_t round0 = (int64_t)blockIdx.x * Q.G;
    PfbUnit<FMT> pf[NPF];
#pragma unroll
    for (int k = 0; k < NPF; ++k)
        if (tid + k * NT < nu) pf[k].load(iq, hend, hv, o + round0 * TB * D - (L - 1) + 4 * (int64_t)(tid + k * NT), Q.n_in);
    for (int g = 0; g < Q.G; ++g) {
        const int64_t m0 = (round0 + g) * TB;
        if (m0 >= Q.n_out) break;
        const int64_t nbase = o + m0 * D - (L - 1);
        if (g == 0) {
#pragma unroll
            for (int k = 0; k < NPF; ++k)
                if (tid + k * NT < nu) pf[k].store(xs + 4 * (tid + k * NT));
            for (int u = tid + NPF * NT; u < nu; u += NT) {   // windows longer than the prefetch depth
                PfbUnit<FMT> t;
                t.load(iq, hend, hv, nbase + 4 * (int64_t)u, Q.n_in);
                t.store(xs + 4 * u);
            }
        }
        __syncthreads();
        if (g + 1 < Q.G) {
#pragma unroll
            for (int k = 0; k < NPF; ++k)
                if (tid + k * NT < nu) pf[k].load(iq, hend, hv, nbase + (int64_t)TB * D + 4 * (int64_t)(tid + k * NT), Q.n_in);
        }
        const int s0 = (int)((m0 * (int64_t)D) % M);
        pfb_stage_a<M1, M2, P, TB>(xs, A, hv_taps, tid, D, dmod, CARRY ? (Q.s_base + s0) % M : s0);
        __syncthreads();
        pfb_pass1<M1, M2>(A, wml, mi, n2);
        __syncthreads();
        // The next round's window lands in LDS here, BEFORE this round's stores are issued: loads and stores
        // share vmcnt and retire out of order with respect to each other, so waiting for a load while
        // stores are in flight means waiting for every store acknowledgement.
        if (g + 1 < Q.G) {
#pragma unroll
            for (int k = 0; k < NPF; ++k)
                if (tid + k * NT < nu) pf[k].store(xs + 4 * (tid + k * NT));
            for (int u = tid + NPF * NT; u < nu; u += NT) {
                PfbUnit<FMT> t;
                t.load(iq, hend, hv, nbase + (int64_t)TB * D + 4 * (int64_t)u, Q.n_in);
                t.store(xs + 4 * u);
            }
        }
        if (tid < TB * M1) pfb_pass2<M1, M2>(A, out, out_stride, m0, Q.n_out, k1b, mib);
    }
}

// ---- carried state of tdm_channeliser -----------------------------------------------------------------
// The next history of every stream after a push (chan_stream.hpp chan_hist_source): slot j of new_h = the last L-1 samples
// of (old_h || this push), copied in wire format (W: uint16_t for cu8 / cs8, uint32_t for cs16, uint2 for cf32).  old_h and new_h are two
// different buffers, so a push shorter than L-1 never shifts a buffer onto itself.  grid.y = stream; strides in samples.
template <typename W>
__global__ __launch_bounds__(256) void k_pfb_hist(const W *__restrict__ iq, int64_t in_stride, const W *__restrict__ old_h,
                                                  W *__restrict__ new_h, int64_t hist_stride, int64_t n_in, int L)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= L - 1) return;
    const int64_t y = blockIdx.y;
    const int64_t src = chan_hist_source(j, n_in, L);
    new_h[y * hist_stride + j] = src >= 0 ? iq[y * in_stride + src] : old_h[y * hist_stride + (-1 - src)];
}

// (Round 4 also built a half-tile variant for the 8-bit formats -- fp16 window, branch sums fused with a radix-2 split of pass 1,
// 80 KB of LDS, two workgroups per compute unit: correct, 0.335 ms against this kernel's 0.237 -- and round 5 one with 16 output
// times per round: 0.340.  Both removed from the source in round 6; docs/HISTORY.md A.2, profiles/r04r_*.)

}  // namespace tdm
