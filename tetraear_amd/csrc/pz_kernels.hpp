// Parallel-form zero-phase decimator: the block kernel body of scipy.signal.decimate as the reference
// calls it (processor.py:254: cheby1(8, 0.05, 0.8/q) run forward and backward, then [::q]).
//
// The composite operator H(z)H(1/z) is evaluated as its partial-fraction expansion (pz_tables.hpp):
// per conjugate pole pair one CAUSAL and one ANTICAUSAL all-pole biquad, both fed by the input
// samples themselves,
//         w[n]  = x[n] - a1 w[n-1]  - a2 w[n-2]          (left to right)
//         w'[n] = x[n] - a1 w'[n+1] - a2 w'[n+2]         (right to left)
//         y[n]  = dx x[n] + sum_pairs  b0 (w[n] + w'[n]) + b1 (w[n-1] + w'[n+1]),
// and y is formed only at the decimated positions.  That is 2 multiply-adds per real sample, pair and
// direction (32 per complex sample for the order-8 filter) against 64 operations for the two cascade
// passes, and the blocked evaluation needs its start-state corrections only at the S outputs of a lane
// instead of at every sample.  Block structure, cross-block carries and the consumer-side fix-up
// (y = y0 + T1.Gf + T2.Hb) are those of the cascade engine (zp_common.hpp / zp_kernels.hpp).
//
// Geometry: a lane owns L = S*Q consecutive samples, Q = decimation factor, so every lane's outputs sit at
// its local positions 0, Q, 2Q, ... (compile-time); a wavefront owns a block of 64 lanes.
#pragma once
#include <type_traits>

#include "zp_kernels.hpp"
#include "pz_tables.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define TDM_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define TDM_SCHED_FENCE()
#endif
// one sample step of all chains at a time: keeps the scheduler from hoisting the independent halves of later
// steps (and their operands) far ahead, which costs more registers than the file has
#define TDM_STEP_FENCE() TDM_SCHED_FENCE()
// makes a value's computation happen here in program order (the instruction selector otherwise defers the output
// accumulations to the end of the kernel and keeps their operands alive, which spills)
#if defined(__HIP_DEVICE_COMPILE__)
#define TDM_PIN(x) asm volatile("" : "+v"(x))
#else
#define TDM_PIN(x)
#endif

namespace tdm {

// ------------------------------------------------------------------------------------------
// Loader with the wire format as a run-time switch (one kernel per Q instead of one per Q x format):
// gives a lane its L samples of the padded, odd-extended signal, UNSCALED.
//   interior lanes : dword loads (8-bit formats need only 4-byte alignment), converted in registers
//   edge lanes     : (odd extension / zero pad; at most kSlots lanes of the first and last block) a rolled
//                    per-sample loop through a small LDS buffer -- no stack array, no scratch
// ------------------------------------------------------------------------------------------
struct alignas(4) u32x4_a4 {
    uint32_t x, y, z, w;
};
struct alignas(8) f64x2_a8 {
    double x, y;
};
struct alignas(4) f32x2_a4 {
    float x, y;
};

template <int L, int EDGE>
struct PzEdgeGeom {
    static constexpr int P0 = (L - EDGE % L) % L;
    static constexpr int kHead = (P0 + EDGE) / L;              // lanes of block 0 before signal sample 0
    static constexpr int kTail = 1 + (EDGE + L - 2) / L;       // lanes that hold the tail extension
    static constexpr int kSlots = kHead + kTail;
    static constexpr int kDoubles = kSlots * L * 2;
};

template <bool SHIFT>
struct RawLoaderRT {
    const void *iq;            // first sample of row 0
    int64_t row_stride;        // samples between rows (0 = shared stream)
    const double *pre_shift;   // per row [Hz] or null: frequency_shift of the stream on load (processor.py:85-100)
    double fs;
    int32_t fmt;
    // fast_shift != 0: the pre-shift's phase as the IDEAL ramp from an exactly anchored first sample of the lane (8
    // instructions per sample) instead of the reference's own rounding of theta_j = fl(ci * fl(j / fs)) reproduced sample
    // by sample (29).  The two differ by the reference's rounding of theta: up to 6e-11 rad at 787.5 kHz x 0.1 s -- soft
    // symbols within 1e-9 instead of 1e-10, and a hard decision can differ only where its margin is below that (the
    // per-carrier min_margin output says so; tetrahip.h tdm_plan_option "fast_pre_shift").
    int32_t fast_shift;
    // rows_per_chunk > 1 (tdm_plan_option "rows_per_chunk"): that many consecutive plan rows read the SAME input row --
    // C carriers shifted out of each of T consecutive chunks of one stream in one call (plan rows = T x C)
    int32_t rows_per_chunk;

    TDM_HD int bytes() const { return wire_bytes(fmt); }
    TDM_HD const void *row_ptr(int row) const { return (const char *)iq + (int64_t)(rows_per_chunk > 1 ? row / rows_per_chunk : row) * row_stride * bytes(); }
    TDM_HD double row_shift(int row) const { return (SHIFT && pre_shift) ? pre_shift[row] : 0.0; }

    TDM_HD void raw(const void *rowp, int64_t k, double &re, double &im) const
    {
        wire_dispatch(fmt, [&](auto F) TDM_WIRE_INLINE { convert_one<decltype(F)::value>(rowp, k, re, im); });
    }
    TDM_HD void sample(const void *rowp, int64_t k, double f, double &re, double &im) const
    {
        raw(rowp, k, re, im);
        if (SHIFT && f != 0.0) nco_rotate(re, im, k, f, fs);
    }
    // sample e of the odd extension of the row (scipy odd_ext, _arraytools.py), zero outside it
    TDM_HD void ext_sample(const void *rowp, double f, int64_t e, int64_t n, int edge, double &re, double &im) const
    {
        re = 0;
        im = 0;
        if (e < 0 || e >= n + 2 * (int64_t)edge) return;
        if (e < edge) {  // 2*x[0] - x[edge - e]
            double ar, ai;
            sample(rowp, 0, f, ar, ai);
            sample(rowp, edge - e, f, re, im);
            re = 2 * ar - re;
            im = 2 * ai - im;
        } else if (e < edge + n) {
            sample(rowp, e - edge, f, re, im);
        } else {  // 2*x[n-1] - x[n-2-(e-edge-n)]
            double ar, ai;
            sample(rowp, n - 1, f, ar, ai);
            sample(rowp, n - 2 - (e - edge - n), f, re, im);
            re = 2 * ar - re;
            im = 2 * ai - im;
        }
    }

    template <int L, int FMT>
    TDM_HD void fast8(const char *p, double *xr, double *xi) const
    {
        // 8-bit pairs: 2L bytes
        if ((((uintptr_t)p) & 3) == 0) {
            constexpr int NQ = (2 * L) / 16, NDW = ((2 * L) % 16) / 4;
            uint32_t w[(2 * L + 3) / 4];
            const u32x4_a4 *v = (const u32x4_a4 *)p;
#pragma unroll
            for (int c = 0; c < NQ; ++c) {
                const u32x4_a4 t = v[c];
                w[4 * c] = t.x; w[4 * c + 1] = t.y; w[4 * c + 2] = t.z; w[4 * c + 3] = t.w;
            }
            const uint32_t *d = (const uint32_t *)(p + 16 * NQ);
#pragma unroll
            for (int c = 0; c < NDW; ++c) w[4 * NQ + c] = d[c];
            if ((2 * L) % 4) w[(2 * L) / 4] = *(const uint16_t *)(p + (2 * L) / 4 * 4);
#pragma unroll
            for (int i = 0; i < L; ++i) {
                const uint32_t s = w[i / 2] >> (16 * (i % 2));
                wire_f64_bytes<FMT>(s & 255u, (s >> 8) & 255u, xr[i], xi[i]);
            }
        } else {
            const uint16_t *h = (const uint16_t *)p;
#pragma unroll
            for (int i = 0; i < L; ++i) {
                const uint32_t s = h[i];
                wire_f64_bytes<FMT>(s & 255u, (s >> 8) & 255u, xr[i], xi[i]);
            }
        }
    }

    // x[i] = padded-ext sample seg + i (zero outside the extended signal)
    template <int L, int EDGE, class Comm>
    TDM_HD void load(Comm &cm, int row, int blk, int lane, const ZpParams &P, double *xr, double *xi) const
    {
        typedef PzEdgeGeom<L, EDGE> G;
        const int64_t seg = (int64_t)blk * (kWave * L) + (int64_t)lane * L;
        const void *rowp = row_ptr(row);
        const double f = row_shift(row);
        const int64_t n = P.n;
        const int64_t e0 = seg - G::P0;  // ext index of x[0]
        if (e0 >= EDGE && e0 + L <= EDGE + n) {
            const int64_t k = e0 - EDGE;
            const char *p = (const char *)rowp + k * bytes();
            // frequency_shift of the shared stream with a running phasor over the lane's consecutive samples; the
            // anchor's (out-of-line) sincos runs before the samples occupy the register file
            NcoRunT<1> nco;
            if (SHIFT && f != 0.0) {
                if (fast_shift) {
                    const phasor a = nco_phasor(k, f, fs);   // (the anchor is exact: the reference's own theta_k)
                    nco.ar = a.c;
                    nco.ai = a.s;
                } else {
                    nco.init(k, f, fs);
                }
            }
            // (spelled out, not wire_dispatch: the order in which the compiler lays these five bodies out decides
            // k_pz_block's register allocation -- at 256 VGPRs, its spills -- and through the dispatcher it comes out another)
            switch (fmt) {
            case FMT_CU8: fast8<L, FMT_CU8>(p, xr, xi); break;
            case FMT_CS8: fast8<L, FMT_CS8>(p, xr, xi); break;
            case FMT_CF32: {
                const f32x2_a4 *v = (const f32x2_a4 *)p;
#pragma unroll
                for (int i = 0; i < L; ++i) {
                    const f32x2_a4 t = v[i];
                    xr[i] = (double)t.x;
                    xi[i] = (double)t.y;
                }
            } break;
            case FMT_CS16: {   // one word per sample (int16 I low, Q high), rows are 4-byte aligned: 16-byte loads of 4 samples
                constexpr int NQ = L / 4;
                const u32x4_a4 *v = (const u32x4_a4 *)p;
                uint32_t w[L];
#pragma unroll
                for (int c = 0; c < NQ; ++c) {
                    const u32x4_a4 t = v[c];
                    w[4 * c] = t.x; w[4 * c + 1] = t.y; w[4 * c + 2] = t.z; w[4 * c + 3] = t.w;
                }
#pragma unroll
                for (int i = 4 * NQ; i < L; ++i) w[i] = ((const uint32_t *)p)[i];
#pragma unroll
                for (int i = 0; i < L; ++i) wire_f64<FMT_CS16>(w[i], xr[i], xi[i]);
            } break;
            default: {
                const f64x2_a8 *v = (const f64x2_a8 *)p;
#pragma unroll
                for (int i = 0; i < L; ++i) {
                    const f64x2_a8 t = v[i];
                    xr[i] = t.x;
                    xi[i] = t.y;
                }
            } break;
            }
            if (SHIFT && f != 0.0 && fast_shift) {
                // ideal ramp: p_{i+1} = p_i W, W = exp(i ci / fs), from the lane's exactly anchored first sample
                double wr, wi;
                sincos(-(2.0 * M_PI) * f / fs, &wi, &wr);
                double c = nco.ar, sn = nco.ai;
#pragma unroll
                for (int i = 0; i < L; ++i) {
                    const double a = xr[i], b = xi[i];
                    xr[i] = a * c - b * sn;
                    xi[i] = a * sn + b * c;
                    const double nc = c * wr - sn * wi, ns = c * wi + sn * wr;
                    c = nc;
                    sn = ns;
                }
            } else if (SHIFT && f != 0.0) {
#pragma unroll
                for (int i = 0; i < L; ++i) {
                    double c = nco.ar, sn = nco.ai;
                    if (i > 0) nco.next(f, fs, c, sn);
                    const double a = xr[i], b = xi[i];
                    xr[i] = a * c - b * sn;
                    xi[i] = a * sn + b * c;
#if defined(__HIP_DEVICE_COMPILE__)
                    __builtin_amdgcn_sched_barrier(0);
#endif
                }
            }
        } else if (e0 >= n + 2 * (int64_t)EDGE) {
#pragma unroll
            for (int i = 0; i < L; ++i) { xr[i] = 0; xi[i] = 0; }
        } else {
            int slot;
            if (e0 < EDGE) {
                slot = (int)(seg / L);
            } else {
                const int64_t seg_t0 = ((G::P0 + EDGE + n) / L) * L;
                slot = G::kHead + (int)((seg - seg_t0) / L);
            }
            double *buf = cm.edge_slots() + (size_t)slot * L * 2;
#pragma unroll 1
            for (int i = 0; i < L; ++i) {
                double re, im;
                ext_sample(rowp, f, e0 + i, n, EDGE, re, im);
                buf[2 * i] = re;
                buf[2 * i + 1] = im;
            }
#pragma unroll
            for (int i = 0; i < L; ++i) { xr[i] = buf[2 * i]; xi[i] = buf[2 * i + 1]; }
        }
    }
};

// ------------------------------------------------------------------------------------------
// Block body: one wavefront = one block of 64 lanes x L samples, L = Q*S.
//   Comm: edge_slots() -> PzEdgeGeom<L,EDGE>::kDoubles doubles of wavefront-private scratch (pz_raw_body: PzRawScratch);
//   shfl_up2<2> / shfl_down2<2> as in zp_block_body.
// ------------------------------------------------------------------------------------------
// The second row-total step of a pair whose multiply by C^(16 L) is left out: only the row next to the source lane takes
// the total (row 2 <- lane 31, row 1 <- lane 32), the row beyond it takes 0 like the rows that never had a source.  A Comm
// that says kRowTotalNear does that in the shuffle itself; any other gets the ordinary shuffle and a select.
template <class Comm, class = void>
struct PzCommRowTotalNear { static constexpr bool value = false; };
template <class Comm>
struct PzCommRowTotalNear<Comm, std::void_t<decltype(Comm::kRowTotalNear)>> { static constexpr bool value = Comm::kRowTotalNear; };

template <class Comm>
TDM_HD void pz_row_total_near2(Comm &cm, int lane, const double *zr, const double *zq, double *jr, double *jq, const double *ur,
                               const double *uq, double *kr, double *kq)
{
    if constexpr (PzCommRowTotalNear<Comm>::value) {
        cm.template row_total_prev2_near<2>(zr, zq, jr, jq);
        cm.template row_total_next2_near<2>(ur, uq, kr, kq);
    } else {
        cm.template row_total_prev2<2>(zr, zq, jr, jq, 1);
        cm.template row_total_next2<2>(ur, uq, kr, kq, 1);
        const bool far_f = lane >= 48, far_b = lane < 16;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            jr[k] = far_f ? 0.0 : jr[k]; jq[k] = far_f ? 0.0 : jq[k];
            kr[k] = far_b ? 0.0 : kr[k]; kq[k] = far_b ? 0.0 : kq[k];
        }
    }
}

// Phases 2 and 3 of a block, shared by the kernels that differ in how a lane holds its samples: scans of the lane
// end states, exports of the block's end states, start-state responses at the lane's outputs, block-local outputs
// (minus `y_const`: the response to a constant input offset that a kernel working on raw integers leaves out).
// Keep::kept(s): the scan terms pair s keeps (pz_tables.hpp PzScanKeep; PzScanKeepAll: every term).  A term that is left
// out is not there at all -- no shuffle, no table load, no multiply-add --; a kept one has the operands and the place it
// has with every term kept.
// BLOCK_STORE_TEST: the S outputs of a lane are stored under ONE wave-uniform test where the whole block lies inside the
// row (every block but a row's first and last ones) instead of under S per-output tests; the values stored are the same.
// The raw-integer kernel asks for it; the double-based one keeps the per-output tests it always had.
template <int Q, int S, int EDGE, class Keep = PzScanKeepAll, bool BLOCK_STORE_TEST = false, class Comm>
TDM_HD void pz_block_finish(const ZpParams &P, Comm &cm, int lane, int blk, int row, double (*zr)[2], double (*zq)[2],
                            double (*ur)[2], double (*uq)[2], double *yr, double *yi, double y_const)
{
    constexpr int NP = PzLayout::kMaxPairs, D = 2 * NP;
    constexpr int L = Q * S;
    constexpr int Bn = kWave * L;
    typedef PzEdgeGeom<L, EDGE> G;
    const int64_t nbD = (int64_t)P.nb * D;
    double *Ef = P.Ef + ((int64_t)row * nbD + (int64_t)blk * D) * 2;
    double *Eb = P.Eb + ((int64_t)row * nbD + (int64_t)blk * D) * 2;
    const bool last_blk = (blk == P.nb - 1);
    // ---------------- phase 2: inclusive scans of the lanes' end states ----------------
    // I_l = e_l + C^L I_{l -/+ 1}, all pairs and both directions per step (eight independent scans share each step's
    // latency).  The shuffles follow the hardware's lane rows: four Kogge-Stone steps inside each row of 16 lanes
    // (DPP row shifts, no LDS traffic), then the row totals are passed on twice (rows 1,3 <- 0,2; rows 2,3 <- lane
    // 31), where the distance to the source lane -- hence the transition matrix -- depends on the lane.
    double lmf[NP][4], lmb[NP][4];   // C^(L (r+1)) for this lane's distance to the previous / next row
    {
        const int r = lane & 15;
        const f64x2 *tf = (const f64x2 *)(P.pz + PzLayout::off_rowm(S)) + (size_t)r * NP * 2;
        const f64x2 *tb = (const f64x2 *)(P.pz + PzLayout::off_rowm(S)) + (size_t)(15 - r) * NP * 2;
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            const f64x2 a0 = tf[s * 2], a1 = tf[s * 2 + 1], c0 = tb[s * 2], c1 = tb[s * 2 + 1];
            lmf[s][0] = a0.x; lmf[s][1] = a0.y; lmf[s][2] = a1.x; lmf[s][3] = a1.y;
            lmb[s][0] = c0.x; lmb[s][1] = c0.y; lmb[s][2] = c1.x; lmb[s][3] = c1.y;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = 1 << j;
        double jr[NP][2], jq[NP][2], kr[NP][2], kq[NP][2];
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            if (Keep::kept(s) <= j) continue;
            cm.template row_shr2<2>(zr[s], zq[s], jr[s], jq[s], d);   // lane - d of the same row, 0 where there is none
            cm.template row_shl2<2>(ur[s], uq[s], kr[s], kq[s], d);   // lane + d
        }
        const double *Mj = P.Mpow + j * 4;
        TDM_OPAQUE_SPTR(Mj);
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            if (Keep::kept(s) <= j) continue;
            const auto M = TDM_CPTR(Mj + (size_t)s * kScanSteps * 4);
            const double m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3];
            zr[s][0] = fma(m0, jr[s][0], fma(m1, jr[s][1], zr[s][0]));
            zr[s][1] = fma(m2, jr[s][0], fma(m3, jr[s][1], zr[s][1]));
            zq[s][0] = fma(m0, jq[s][0], fma(m1, jq[s][1], zq[s][0]));
            zq[s][1] = fma(m2, jq[s][0], fma(m3, jq[s][1], zq[s][1]));
            ur[s][0] = fma(m0, kr[s][0], fma(m1, kr[s][1], ur[s][0]));
            ur[s][1] = fma(m2, kr[s][0], fma(m3, kr[s][1], ur[s][1]));
            uq[s][0] = fma(m0, kq[s][0], fma(m1, kq[s][1], uq[s][0]));
            uq[s][1] = fma(m2, kq[s][0], fma(m3, kq[s][1], uq[s][1]));
        }
        TDM_SCHED_FENCE();
    }
#pragma unroll
    for (int step = 0; step < 2; ++step) {
        double jr[NP][2], jq[NP][2], kr[NP][2], kq[NP][2];
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            if (step == 1 && Keep::kept(s) <= 4) {
                pz_row_total_near2(cm, lane, zr[s], zq[s], jr[s], jq[s], ur[s], uq[s], kr[s], kq[s]);
                continue;
            }
            cm.template row_total_prev2<2>(zr[s], zq[s], jr[s], jq[s], step);   // step 0: rows 1,3 <- lane 15 of rows 0,2; step 1: rows 2,3 <- lane 31
            cm.template row_total_next2<2>(ur[s], uq[s], kr[s], kq[s], step);   // mirror image: rows 0,2 <- lane 0 of rows 1,3; rows 0,1 <- lane 32
        }
        if (step == 1) {
            // rows 3 (causal) and 0 (anticausal) are a whole row further from the source lane: C^(16 L) first
            const double *M16 = P.Mpow + 4 * 4;
            TDM_OPAQUE_SPTR(M16);
#pragma unroll
            for (int s = 0; s < NP; ++s) {
                if (Keep::kept(s) <= 4) continue;
                const auto M = TDM_CPTR(M16 + (size_t)s * kScanSteps * 4);
                const double m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3];
                const bool far_f = lane >= 48, far_b = lane < 16;
                const double a0 = fma(m0, jr[s][0], m1 * jr[s][1]), a1 = fma(m2, jr[s][0], m3 * jr[s][1]);
                const double b0_ = fma(m0, jq[s][0], m1 * jq[s][1]), b1_ = fma(m2, jq[s][0], m3 * jq[s][1]);
                jr[s][0] = far_f ? a0 : jr[s][0]; jr[s][1] = far_f ? a1 : jr[s][1];
                jq[s][0] = far_f ? b0_ : jq[s][0]; jq[s][1] = far_f ? b1_ : jq[s][1];
                const double c0 = fma(m0, kr[s][0], m1 * kr[s][1]), c1 = fma(m2, kr[s][0], m3 * kr[s][1]);
                const double d0_ = fma(m0, kq[s][0], m1 * kq[s][1]), d1_ = fma(m2, kq[s][0], m3 * kq[s][1]);
                kr[s][0] = far_b ? c0 : kr[s][0]; kr[s][1] = far_b ? c1 : kr[s][1];
                kq[s][0] = far_b ? d0_ : kq[s][0]; kq[s][1] = far_b ? d1_ : kq[s][1];
            }
        }
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            zr[s][0] = fma(lmf[s][0], jr[s][0], fma(lmf[s][1], jr[s][1], zr[s][0]));
            zr[s][1] = fma(lmf[s][2], jr[s][0], fma(lmf[s][3], jr[s][1], zr[s][1]));
            zq[s][0] = fma(lmf[s][0], jq[s][0], fma(lmf[s][1], jq[s][1], zq[s][0]));
            zq[s][1] = fma(lmf[s][2], jq[s][0], fma(lmf[s][3], jq[s][1], zq[s][1]));
            ur[s][0] = fma(lmb[s][0], kr[s][0], fma(lmb[s][1], kr[s][1], ur[s][0]));
            ur[s][1] = fma(lmb[s][2], kr[s][0], fma(lmb[s][3], kr[s][1], ur[s][1]));
            uq[s][0] = fma(lmb[s][0], kq[s][0], fma(lmb[s][1], kq[s][1], uq[s][0]));
            uq[s][1] = fma(lmb[s][2], kq[s][0], fma(lmb[s][3], kq[s][1], uq[s][1]));
        }
        TDM_SCHED_FENCE();
    }
    // ---------------- phase 3: exports; start-state responses at the lane's outputs ----------------
#pragma unroll
    for (int s = 0; s < NP; ++s) {
        if (lane == kWave - 1) {
            Ef[(2 * s) * 2] = zr[s][0]; Ef[(2 * s) * 2 + 1] = zq[s][0];
            Ef[(2 * s + 1) * 2] = zr[s][1]; Ef[(2 * s + 1) * 2 + 1] = zq[s][1];
        }
        if (lane == 0) {
            Eb[(2 * s) * 2] = ur[s][0]; Eb[(2 * s) * 2 + 1] = uq[s][0];
            Eb[(2 * s + 1) * 2] = ur[s][1]; Eb[(2 * s + 1) * 2 + 1] = uq[s][1];
        }
        if (last_blk && lane == (P.len_last - 1) / L) {
            // the lane holding the last extended sample: its causal state after the lane's (zero-padded) tail
            double *El = P.Elast + (int64_t)row * D * 2;
            El[(2 * s) * 2] = zr[s][0]; El[(2 * s) * 2 + 1] = zq[s][0];
            El[(2 * s + 1) * 2] = zr[s][1]; El[(2 * s + 1) * 2 + 1] = zq[s][1];
        }
    }
    {
        // start states of this lane = inclusive values of the neighbour lanes (0 at the ends of the block)
        double sr[NP][2], sq[NP][2], tr[NP][2], tq[NP][2];
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            cm.template wave_shr1<2>(zr[s], zq[s], sr[s], sq[s]);
            cm.template wave_shl1<2>(ur[s], uq[s], tr[s], tq[s]);
        }
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            const double *zfs = P.pz + PzLayout::off_zf + s * S * 2;
            const double *zbs = P.pz + PzLayout::off_zf + (NP + s) * S * 2;   // == off_zb(S) + s*S*2
            TDM_OPAQUE_SPTR(zfs);
            TDM_OPAQUE_SPTR(zbs);
#pragma unroll
            for (int t = 0; t < S; ++t) {
                const double z0 = TDM_CPTR(zfs)[t * 2], z1 = TDM_CPTR(zfs)[t * 2 + 1];
                const double v0 = TDM_CPTR(zbs)[t * 2], v1 = TDM_CPTR(zbs)[t * 2 + 1];
                yr[t] = fma(z0, sr[s][0], fma(z1, sr[s][1], fma(v0, tr[s][0], fma(v1, tr[s][1], yr[t]))));
                yi[t] = fma(z0, sq[s][0], fma(z1, sq[s][1], fma(v0, tq[s][0], fma(v1, tq[s][1], yi[t]))));
                TDM_PIN(yr[t]);
                TDM_PIN(yi[t]);
            }
        }
    }
    // ---------------- block-local outputs: S consecutive decimated samples per lane ----------------
    {
        static_assert((G::P0 + EDGE) % Q == 0 || S == 0, "outputs sit on lane-local multiples of Q");
        const int64_t j0 = ((int64_t)blk * Bn + (int64_t)lane * L - P.k0L) / Q;   // exact: every term is a multiple of Q
        f64x2 *y0 = (f64x2 *)(P.y0 + (int64_t)row * P.n_out * 2);
        // (one test for the wavefront: only block 0 has lanes before the row's first output, only a row's last block(s) a
        //  lane whose outputs cross n_out)
        const bool all_inside = BLOCK_STORE_TEST && (int64_t)blk * Bn >= P.k0L && ((int64_t)(blk + 1) * Bn - P.k0L) / Q <= P.n_out;
        if (all_inside) {
#pragma unroll
            for (int t = 0; t < S; ++t) y0[j0 + t] = f64x2{yr[t] - y_const, yi[t] - y_const};
        } else if ((int64_t)blk * Bn + (int64_t)lane * L >= P.k0L) {
#pragma unroll
            for (int t = 0; t < S; ++t)
                if (j0 + t < P.n_out) y0[j0 + t] = f64x2{yr[t] - y_const, yi[t] - y_const};
        }
    }
}

template <int Q, int S, int EDGE, class Loader, class Comm>
TDM_HD void pz_block_body(const ZpParams &P, const Loader &ld, Comm &cm, int lane, int blk, int row)
{
    constexpr int NP = PzLayout::kMaxPairs;
    constexpr int L = Q * S;
    typedef PzEdgeGeom<L, EDGE> G;
    double xr[L], xi[L];
    ld.template load<L, EDGE>(cm, row, blk, lane, P, xr, xi);

    const auto pz = TDM_CPTR(P.pz);
    const bool inject = (blk == 0 && lane == 0);
    const double e0r = xr[G::P0], e0i = xi[G::P0];
    const bool last_blk = (blk == P.nb - 1);

    double yr[S], yi[S];
    {
        const double dx = pz[PzLayout::off_dx];
#pragma unroll
        for (int t = 0; t < S; ++t) { yr[t] = dx * xr[t * Q]; yi[t] = dx * xi[t * Q]; }
    }

    // ---------------- phase 1: the recurrences, one pole pair at a time ----------------
    // causal bank left to right, anticausal bank right to left: four independent chains in flight
    // (two directions x re/im).  End states of all pairs are kept for the scans of phase 2.
    double zr[NP][2], zq[NP][2];   // causal end state (w[L-1], w[L-2]), re / im
    double ur[NP][2], uq[NP][2];   // anticausal end state (w'[0], w'[1])
#pragma unroll
    for (int s = 0; s < NP; ++s) {
        const double *cs = P.pz;
        TDM_OPAQUE_SPTR(cs);   // (per-pair scalar loads: keeps all pairs' constants from being fetched at once)
        const double na1 = -TDM_CPTR(cs)[PzLayout::off_a1 + s], na2 = -TDM_CPTR(cs)[PzLayout::off_a2 + s];
        const double b0 = TDM_CPTR(cs)[PzLayout::off_b0 + s], b1 = TDM_CPTR(cs)[PzLayout::off_b1 + s];
        double f1r = 0, f2r = 0, f1q = 0, f2q = 0;   // causal (w[n-1], w[n-2]), re / im
        double a1r = 0, a2r = 0, a1q = 0, a2q = 0;   // anticausal (w'[n+1], w'[n+2])
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const int ib = L - 1 - i;
            if (i == G::P0) {
                // scipy's zi*ext[0]: constant history ext[0] before the first extended sample
                const double g = TDM_CPTR(cs)[PzLayout::off_g + s];
                f1r = inject ? g * e0r : f1r; f2r = inject ? g * e0r : f2r;
                f1q = inject ? g * e0i : f1q; f2q = inject ? g * e0i : f2q;
            }
            {
                const double wr = fma(na1, f1r, fma(na2, f2r, xr[i]));
                const double wq = fma(na1, f1q, fma(na2, f2q, xi[i]));
                if (i % Q == 0) {
                    yr[i / Q] = fma(b0, wr, fma(b1, f1r, yr[i / Q]));
                    yi[i / Q] = fma(b0, wq, fma(b1, f1q, yi[i / Q]));
                    TDM_PIN(yr[i / Q]);
                    TDM_PIN(yi[i / Q]);
                }
                f2r = f1r; f1r = wr;
                f2q = f1q; f1q = wq;
            }
            {
                const double wr = fma(na1, a1r, fma(na2, a2r, xr[ib]));
                const double wq = fma(na1, a1q, fma(na2, a2q, xi[ib]));
                if (ib % Q == 0) {
                    yr[ib / Q] = fma(b0, wr, fma(b1, a1r, yr[ib / Q]));
                    yi[ib / Q] = fma(b0, wq, fma(b1, a1q, yi[ib / Q]));
                    TDM_PIN(yr[ib / Q]);
                    TDM_PIN(yi[ib / Q]);
                }
                a2r = a1r; a1r = wr;
                a2q = a1q; a1q = wq;
            }
        }
        zr[s][0] = f1r; zr[s][1] = f2r; zq[s][0] = f1q; zq[s][1] = f2q;
        ur[s][0] = a1r; ur[s][1] = a2r; uq[s][0] = a1q; uq[s][1] = a2q;
        TDM_PIN(zr[s][0]); TDM_PIN(zr[s][1]); TDM_PIN(zq[s][0]); TDM_PIN(zq[s][1]);
        TDM_PIN(ur[s][0]); TDM_PIN(ur[s][1]); TDM_PIN(uq[s][0]); TDM_PIN(uq[s][1]);
        TDM_SCHED_FENCE();
    }
    pz_block_finish<Q, S, EDGE>(P, cm, lane, blk, row, zr, zq, ur, uq, yr, yi, 0.0);
    // the last extended sample (the anticausal start needs it, see pz_carry_last): 2 x[n-1] - x[n-1-edge]
    if (last_blk && lane == 0) {
        double re, im;
        ld.ext_sample(ld.row_ptr(row), ld.row_shift(row), P.n + 2 * (int64_t)EDGE - 1, P.n, EDGE, re, im);
        P.flast[(int64_t)row * 2] = re;
        P.flast[(int64_t)row * 2 + 1] = im;
    }
}

// ------------------------------------------------------------------------------------------
// The same block for 8-bit wire formats with the samples kept as the raw integers (round-2 main kernel): a lane then
// holds four times as many samples in the same registers (L = Q*S = 120 at q = 10), so the per-block work -- scans,
// start-state responses -- is spread over four times as many samples.  The recurrences run on the integers
// themselves (exactly representable); the wire format's affine map x = c*u - o (cu8: c = fl(1/127.5), o = 1; cs8:
// c = 2^-7, o = 0) is applied through linearity: c is folded into the output taps and tables by the host
// (build_pz_tables in_scale) and the response to the constant -o over the extended row, which scipy's edge recipe makes
// exactly -o*H(1)^2 at every output, is subtracted from the block-local outputs.  Against the reference's own
// two-rounding conversion this moves an input sample by at most one ulp of 1.0, far below the arithmetic's own noise.
// Each sample is converted once per direction (cheap: byte -> f32 -> f64).
//   WIDE = false : interior blocks, two samples per dword as they come off the wire
//   WIDE = true  : the first block and the block(s) holding the tail extension: samples as int16 pairs, because the odd
//                  extension 2 u[0] - u[k] does not fit a byte; the lanes holding extension or pad samples read theirs from a
//                  small LDS buffer that the whole wavefront fills (pz_raw_fill_edges)
// ------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
#define TDM_OPAQUE_V(x) asm volatile("" : "+v"(x))
#define TDM_PIN_S(x) asm volatile("" : "+s"(x))   // a scalar-loaded value has to have arrived here
#else
#define TDM_OPAQUE_V(x)
#define TDM_PIN_S(x)
#endif
// OPAQUE: the second conversion of a sample (other direction, many steps later) must not be recognised as the same
// computation -- the compiler would keep the first result alive across the loop instead of converting again
// The bias of the raw-integer kernel's samples (round 6).  4096 + u, u a byte, is exactly the double whose high dword is
// 0x40B00000 | u << 8 and whose low dword is zero: byte 1 of the high dword IS the sample.  So a cu8 sample becomes an fp64
// operand by ONE byte permute (v_perm_b32) into the high half of a register pair whose low half stays zero and whose high
// half keeps its 0x40B0 -- against a bit-field extract plus a conversion (two instructions at the fp64 issue cost each:
// 1012 of the ~7200 vector instructions per lane).  The kernel therefore filters u + 4096; the constant rides out by the
// linearity that already carries the wire format's "- 1": the host folds it into PzLayout::off_yc
// (in_offset = 1 + 4096 * fl(1/127.5), ref_plan.hpp).  Price: the constant part of every state is 33 times larger (DC 4224
// instead of 127.5), i.e. five bits of the 53 go to it; the soft symbols stay within 1e-12 of the reference's.
template <int FMT8>
struct PzRawBias { static constexpr int value = FMT8 == FMT_CU8 ? kPzRawBiasCu8 : 0; };

// a standing operand pair of the permute conversion: 4096.0 = (0x40B00000, 0), opaque to the compiler from here on
TDM_HD void pz_raw_slot_init(double &x)
{
    x = 4096.0;
    TDM_OPAQUE_V(x);
}

#if defined(__HIP_DEVICE_COMPILE__)
// byte BYTE of w into byte 1 of the slot's high dword (selector bytes: 7, 6 = the slot's own 0x40, 0xB0; BYTE; 0x0c = zero).
// volatile: never merged with the other direction's conversion of the same byte, which would keep 240 converted values
// alive across the loop
template <int BYTE>
__device__ __forceinline__ void pz_raw_perm(double &slot, uint32_t w)
{
    uint32_t hi = (uint32_t)__double2hiint(slot);
    constexpr uint32_t sel = (7u << 24) | (6u << 16) | ((uint32_t)BYTE << 8) | 0x0cu;
    asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(hi) : "v"(w), "s"(sel));
    slot = __hiloint2double((int)hi, __double2loint(slot));
}
#endif

// re / im are IN-OUT for the 8-bit unsigned narrow form on the device: standing slots made by pz_raw_slot_init
template <int FMT8, bool WIDE, bool OPAQUE>
TDM_HD void pz_raw_cvt(const uint32_t *raw, int i, double &re, double &im)
{
    if (WIDE) {
        // (int16 pairs; in-row samples were packed with the bias on)
        uint32_t w = raw[i];
        if (OPAQUE) TDM_OPAQUE_V(w);
        re = (double)(int32_t)(int16_t)(w & 0xffffu);
        im = (double)((int32_t)w >> 16);
    } else {
        const uint32_t w = raw[i / 2];
#if defined(__HIP_DEVICE_COMPILE__)
        if (OPAQUE) {
            if (FMT8 == FMT_CU8) {
                if (i % 2 == 0) { pz_raw_perm<0>(re, w); pz_raw_perm<1>(im, w); }
                else { pz_raw_perm<2>(re, w); pz_raw_perm<3>(im, w); }
            } else {
                // the byte comes out of its dword by a bit-field extract written as volatile asm (see pz_raw_perm)
                uint32_t br, bi;
                if (i % 2 == 0) {
                    asm volatile("v_bfe_i32 %0, %1, 0, 8" : "=v"(br) : "v"(w));
                    asm volatile("v_bfe_i32 %0, %1, 8, 8" : "=v"(bi) : "v"(w));
                } else {
                    asm volatile("v_bfe_i32 %0, %1, 16, 8" : "=v"(br) : "v"(w));
                    asm volatile("v_bfe_i32 %0, %1, 24, 8" : "=v"(bi) : "v"(w));
                }
                re = (double)(int32_t)br;
                im = (double)(int32_t)bi;
            }
            return;
        }
#endif
        const int sh = 16 * (i % 2);
        if (FMT8 == FMT_CU8) {
            re = (double)(int)(((w >> sh) & 0xffu) + (uint32_t)PzRawBias<FMT8>::value);
            im = (double)(int)(((w >> (sh + 8)) & 0xffu) + (uint32_t)PzRawBias<FMT8>::value);
        } else {
            re = (double)(int32_t)(int8_t)((w >> sh) & 0xffu);
            im = (double)(int32_t)(int8_t)((w >> (sh + 8)) & 0xffu);
        }
    }
}

// integer sample k of the row (re, im)
template <int FMT8>
TDM_HD void pz_raw_sample(const void *rowp, int64_t k, int &re, int &im)
{
    if (FMT8 == FMT_CU8) {
        const uint8_t *p = (const uint8_t *)rowp + 2 * k;
        re = p[0];
        im = p[1];
    } else {
        const int8_t *p = (const int8_t *)rowp + 2 * k;
        re = p[0];
        im = p[1];
    }
}

// ------------------------------------------------------------------------------------------
// Phase 1 of a narrow block in the FOLDED form: the banks are stepped only at the output rate.  A window of Q samples
// W_j = x[Q t + 1 + j] moves the causal state v = (w[n], w[n-1]) from n = Q t to Q t + Q and the anticausal state
// u[t] = (w'[Q t + 1], w'[Q t + 2]) from u[t + 1] to u[t]:
//     v[Q t + Q] = M v[Q t] + sum_j gamma_{Q-1-j} W_j,      u[t] = M u[t + 1] + sum_j gamma_j W_j,      M = C^Q.
// Both banks have the same poles, so the two sums are mirror images: with s_j = W_j + W_{Q-1-j}, d_j = W_j - W_{Q-1-j}
// (exact on the integers) and the host's folded coefficients (PzLayout::off_fold)
//     S = sum_{j < Q/2} (gamma_j + gamma_{Q-1-j})/2 s_j,   A = sum_{j < Q/2} (gamma_j - gamma_{Q-1-j})/2 d_j,
// the anticausal sum is S + A and the causal one S - A: Q multiply-adds per state component for both directions, against
// 2 Q for the per-sample recurrences, and a byte is converted once.  The windows are taken in ascending order, once.  The
// anticausal states, which chain downwards, come per SEGMENT of at most kFoldSeg windows from ascending prefix sums
//     Pf[t] = sum_{t' < t} M^t' G_t'  (G = S + A),      u[t] = M^-t (Pf[n] + M^n u_in - Pf[t]);
// the output takes -(ka^T M^-t) Pf[t] when window t is processed and +(ka^T M^-t) (Pf[n] + M^n u_in) once the later
// segments are known.  M^-t grows like |p|^(-Q t): segments are short to keep that below 2^5 for the fastest pair.
// The lane's samples past the last window and its first sample take plain recurrence steps.  End states leave in the
// per-sample form's representation: (w[L-1], w[L-2]) and (w'[0], w'[1]).
// ------------------------------------------------------------------------------------------
template <int Q>
struct PzRawFold { static constexpr bool value = Q == PzLayout::kFoldQ; };
// The first segment's totals (16 doubles per lane) wait for the end of the lane in the wavefront's LDS scratch
// (Comm::edge_slots(), which a narrow block does not otherwise use): at the last windows the register file holds two
// finished segments' totals, the running prefix, both banks' states, all outputs and a window's sums -- 272 registers.
constexpr int kPzFoldStash = 2 * 2 * PzLayout::kMaxPairs * kWave;
// doubles of wavefront-private scratch behind Comm::edge_slots() that pz_raw_body needs
template <int Q, int S, int EDGE, bool FOLD>
struct PzRawScratch {
    static constexpr int kEdge = PzEdgeGeom<Q * S, EDGE>::kDoubles;
    static constexpr int kDoubles = (FOLD && PzRawFold<Q>::value && kPzFoldStash > kEdge) ? kPzFoldStash : kEdge;
};

template <int Q, int S, int FMT8>
TDM_HD void pz_raw_fold_lane(const ZpParams &P, const uint32_t *raw, double *stash, double (*zr)[2], double (*zq)[2],
                             double (*ur)[2], double (*uq)[2], double *yr, double *yi)
{
    typedef PzLayout LY;
    constexpr int NP = LY::kMaxPairs, L = Q * S, H = Q / 2, NW = S - 1, SEG = LY::kFoldSeg, NSEG = (NW + SEG - 1) / SEG;
    static_assert(Q == LY::kFoldQ && S >= 2, "folded tables exist for this factor only");
    static_assert(NSEG <= 3, "kPzFoldStash holds ONE segment's totals: a longer lane would keep the others' in registers and spill");
    const double *fold = P.pz + LY::off_fold(S);
    const auto pz = TDM_CPTR(P.pz);
    double xfr, xfq, xbr, xbq;
    pz_raw_slot_init(xfr); pz_raw_slot_init(xfq); pz_raw_slot_init(xbr); pz_raw_slot_init(xbq);
    const double dxf = pz[LY::off_fold_dx(S)];   // (the direct term of output t + 1 is formed in window t, from its last sample)
    double vr[NP][2], vq[NP][2];           // causal (w[Q t], w[Q t - 1])
    double pr[NSEG][NP][2], pq[NSEG][NP][2];   // the segments' prefix sums; after a segment's last window its total
    {
        // (slots of its own: a value that stays alive would have the window loop's slots copied at every conversion)
        double x0r, x0q;
        pz_raw_slot_init(x0r); pz_raw_slot_init(x0q);
        pz_raw_cvt<FMT8, false, true>(raw, 0, x0r, x0q);
#pragma unroll
        for (int s = 0; s < NP; ++s) { vr[s][0] = x0r; vr[s][1] = 0; vq[s][0] = x0q; vq[s][1] = 0; }
        yr[0] = dxf * x0r;
        yi[0] = dxf * x0q;
        TDM_PIN(yr[0]); TDM_PIN(yi[0]);   // (every output accumulation is pinned where it stands, see TDM_PIN)
    }
    // The constants of a (window, pair) step come by scalar loads in two parts, each fetched while the part before it
    // computes: A = the pair's folded coefficients (block sums), B = M, the output taps and the segment row (state
    // updates).  Both parts of two pairs do not fit the scalar registers; a part fetched only when it is needed leaves
    // the vector pipe waiting on the scalar cache at every step.
    auto load_a = [&](int s, double *o) {
        const double *cp = fold + s * LY::kFoldStride;
        TDM_OPAQUE_SPTR(cp);   // (opaque: keeps all pairs' constants from being fetched at once)
        const auto c = TDM_CPTR(cp);
#pragma unroll
        for (int k = 0; k < 4 * H; ++k) o[k] = c[k];
    };
    auto load_b = [&](int s, int tl, double *o) {
        const double *cp = fold + s * LY::kFoldStride;
        TDM_OPAQUE_SPTR(cp);
        const auto c = TDM_CPTR(cp);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = c[LY::kfM + k];   // M, causal taps, (anticausal taps: unused here)
        if (tl > 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) o[8 + k] = c[LY::kfSeg + 6 * (tl - 1) + k];
        }
    };
    double ca[4 * H], cb[14];
    load_a(0, ca);
#pragma unroll
    for (int t = 0; t < NW; ++t) {
        const int seg = t / SEG, tl = t % SEG;
        double sr[H], dr[H], sq[H], dq[H];
#pragma unroll
        for (int j = 0; j < H; ++j) {
            pz_raw_cvt<FMT8, false, true>(raw, t * Q + 1 + j, xfr, xfq);
            pz_raw_cvt<FMT8, false, true>(raw, t * Q + Q - j, xbr, xbq);
            if (j == 0) { yr[t + 1] = dxf * xbr; yi[t + 1] = dxf * xbq; TDM_PIN(yr[t + 1]); TDM_PIN(yi[t + 1]); }
            sr[j] = xfr + xbr; dr[j] = xfr - xbr;
            sq[j] = xfq + xbq; dq[j] = xfq - xbq;
        }
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            // ---- part A: the block sums
            // (scalar loads return in any order, so a use waits for ALL that are in flight: this part's constants are
            //  claimed before the next part's are asked for)
#pragma unroll
            for (int k = 0; k < 4 * H; k += 4) TDM_PIN_S(ca[k]);
            load_b(s, tl, cb);
            double S0r = ca[0] * sr[0], S1r = ca[1] * sr[0], A0r = ca[2] * dr[0], A1r = ca[3] * dr[0];
            double S0q = ca[0] * sq[0], S1q = ca[1] * sq[0], A0q = ca[2] * dq[0], A1q = ca[3] * dq[0];
#pragma unroll
            for (int j = 1; j < H; ++j) {
                S0r = fma(ca[4 * j], sr[j], S0r); S1r = fma(ca[4 * j + 1], sr[j], S1r);
                A0r = fma(ca[4 * j + 2], dr[j], A0r); A1r = fma(ca[4 * j + 3], dr[j], A1r);
                S0q = fma(ca[4 * j], sq[j], S0q); S1q = fma(ca[4 * j + 1], sq[j], S1q);
                A0q = fma(ca[4 * j + 2], dq[j], A0q); A1q = fma(ca[4 * j + 3], dq[j], A1q);
            }
            // (no fence between the parts, none inside the window's conversions: measured 0.447 against 0.456 ms with them)
            // ---- part B: outputs at the lane's position Q t, then the two states
            TDM_PIN_S(cb[0]); TDM_PIN_S(cb[4]);
            if (tl > 0) { TDM_PIN_S(cb[8]); TDM_PIN_S(cb[12]); }
            if (s + 1 < NP || t + 1 < NW) load_a((s + 1) % NP, ca);
            yr[t] = fma(cb[4], vr[s][0], fma(cb[5], vr[s][1], yr[t]));
            yi[t] = fma(cb[4], vq[s][0], fma(cb[5], vq[s][1], yi[t]));
            if (tl > 0) {
                yr[t] = fma(-cb[8], pr[seg][s][0], fma(-cb[9], pr[seg][s][1], yr[t]));
                yi[t] = fma(-cb[8], pq[seg][s][0], fma(-cb[9], pq[seg][s][1], yi[t]));
            }
            {
                const double m0 = cb[0], m1 = cb[1], m2 = cb[2], m3 = cb[3];
                const double n0r = fma(m0, vr[s][0], fma(m1, vr[s][1], S0r - A0r)), n1r = fma(m2, vr[s][0], fma(m3, vr[s][1], S1r - A1r));
                const double n0q = fma(m0, vq[s][0], fma(m1, vq[s][1], S0q - A0q)), n1q = fma(m2, vq[s][0], fma(m3, vq[s][1], S1q - A1q));
                vr[s][0] = n0r; vr[s][1] = n1r; vq[s][0] = n0q; vq[s][1] = n1q;
            }
            const double g0r = S0r + A0r, g1r = S1r + A1r, g0q = S0q + A0q, g1q = S1q + A1q;
            if (tl == 0) {
                pr[seg][s][0] = g0r; pr[seg][s][1] = g1r; pq[seg][s][0] = g0q; pq[seg][s][1] = g1q;
            } else {
                const double m0 = cb[10], m1 = cb[11], m2 = cb[12], m3 = cb[13];
                pr[seg][s][0] = fma(m0, g0r, fma(m1, g1r, pr[seg][s][0])); pr[seg][s][1] = fma(m2, g0r, fma(m3, g1r, pr[seg][s][1]));
                pq[seg][s][0] = fma(m0, g0q, fma(m1, g1q, pq[seg][s][0])); pq[seg][s][1] = fma(m2, g0q, fma(m3, g1q, pq[seg][s][1]));
            }
            TDM_PIN(vr[s][0]); TDM_PIN(vr[s][1]); TDM_PIN(vq[s][0]); TDM_PIN(vq[s][1]);
            TDM_PIN(pr[seg][s][0]); TDM_PIN(pr[seg][s][1]); TDM_PIN(pq[seg][s][0]); TDM_PIN(pq[seg][s][1]);
            TDM_PIN(yr[t]); TDM_PIN(yi[t]);
            if (NSEG > 1 && t == SEG - 1) {
                // (stash is the lane's column of a [16][kWave] array: conflict-free, lane-private, no barrier)
                stash[(4 * s + 0) * kWave] = pr[0][s][0]; stash[(4 * s + 1) * kWave] = pr[0][s][1];
                stash[(4 * s + 2) * kWave] = pq[0][s][0]; stash[(4 * s + 3) * kWave] = pq[0][s][1];
            }
            TDM_STEP_FENCE();
        }
    }
    // ---- the last output's causal part; the Q - 1 samples past the last window: causal on from v, anticausal from zero
    double na1[NP], na2[NP];
#pragma unroll
    for (int s = 0; s < NP; ++s) {
        na1[s] = -pz[LY::off_a1 + s];
        na2[s] = -pz[LY::off_a2 + s];
        yr[S - 1] = fma(pz[LY::off_b0 + s], vr[s][0], fma(pz[LY::off_b1 + s], vr[s][1], yr[S - 1]));
        yi[S - 1] = fma(pz[LY::off_b0 + s], vq[s][0], fma(pz[LY::off_b1 + s], vq[s][1], yi[S - 1]));
        TDM_PIN(yr[S - 1]); TDM_PIN(yi[S - 1]);
    }
    TDM_SCHED_FENCE();
    double a1r[NP], a2r[NP], a1q[NP], a2q[NP];
#pragma unroll
    for (int s = 0; s < NP; ++s) { a1r[s] = 0; a2r[s] = 0; a1q[s] = 0; a2q[s] = 0; }
#pragma unroll
    for (int k = 0; k < Q - 1; ++k) {
        pz_raw_cvt<FMT8, false, true>(raw, NW * Q + 1 + k, xfr, xfq);
        pz_raw_cvt<FMT8, false, true>(raw, L - 1 - k, xbr, xbq);
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            const double wr = fma(na1[s], vr[s][0], fma(na2[s], vr[s][1], xfr)), wq = fma(na1[s], vq[s][0], fma(na2[s], vq[s][1], xfq));
            vr[s][1] = vr[s][0]; vr[s][0] = wr; vq[s][1] = vq[s][0]; vq[s][0] = wq;
            const double ar = fma(na1[s], a1r[s], fma(na2[s], a2r[s], xbr)), aq = fma(na1[s], a1q[s], fma(na2[s], a2q[s], xbq));
            a2r[s] = a1r[s]; a1r[s] = ar; a2q[s] = a1q[s]; a1q[s] = aq;
        }
#pragma unroll
        for (int s = 0; s < NP; ++s) { TDM_PIN(vr[s][0]); TDM_PIN(vq[s][0]); TDM_PIN(a1r[s]); TDM_PIN(a1q[s]); }
    }
    TDM_SCHED_FENCE();
    // ---- the segments' totals chained downwards from u[NW] = (a1, a2); the outputs' share of each segment's start vector
    pz_raw_cvt<FMT8, false, true>(raw, 0, xfr, xfq);
#pragma unroll
    for (int s = 0; s < NP; ++s) {
        const double *cp = fold + s * LY::kFoldStride;
        TDM_OPAQUE_SPTR(cp);
        const auto c = TDM_CPTR(cp);
        double u0r = a1r[s], u1r = a2r[s], u0q = a1q[s], u1q = a2q[s];
        yr[S - 1] = fma(c[LY::kfKa], u0r, fma(c[LY::kfKa + 1], u1r, yr[S - 1]));
        yi[S - 1] = fma(c[LY::kfKa], u0q, fma(c[LY::kfKa + 1], u1q, yi[S - 1]));
        TDM_PIN(yr[S - 1]); TDM_PIN(yi[S - 1]);
#pragma unroll
        for (int seg = NSEG - 1; seg >= 0; --seg) {
            const int n = (NW - seg * SEG) < SEG ? (NW - seg * SEG) : SEG;
            const int o = n == SEG ? LY::kfMn : LY::kfSeg + 6 * (n - 1) + 2;
            const double m0 = c[o], m1 = c[o + 1], m2 = c[o + 2], m3 = c[o + 3];
            double t0r = pr[seg][s][0], t1r = pr[seg][s][1], t0q = pq[seg][s][0], t1q = pq[seg][s][1];
            if (NSEG > 1 && seg == 0) {
                t0r = stash[(4 * s + 0) * kWave]; t1r = stash[(4 * s + 1) * kWave];
                t0q = stash[(4 * s + 2) * kWave]; t1q = stash[(4 * s + 3) * kWave];
            }
            const double n0r = fma(m0, u0r, fma(m1, u1r, t0r)), n1r = fma(m2, u0r, fma(m3, u1r, t1r));
            const double n0q = fma(m0, u0q, fma(m1, u1q, t0q)), n1q = fma(m2, u0q, fma(m3, u1q, t1q));
            u0r = n0r; u1r = n1r; u0q = n0q; u1q = n1q;
#pragma unroll
            for (int tl = 0; tl < n; ++tl) {
                const int t = seg * SEG + tl;
                const int ol = tl == 0 ? LY::kfKa : LY::kfSeg + 6 * (tl - 1);
                yr[t] = fma(c[ol], u0r, fma(c[ol + 1], u1r, yr[t]));
                yi[t] = fma(c[ol], u0q, fma(c[ol + 1], u1q, yi[t]));
                TDM_PIN(yr[t]); TDM_PIN(yi[t]);
            }
        }
        // u[0] = (w'[1], w'[2]): one step to the lane's first sample
        zr[s][0] = vr[s][0]; zr[s][1] = vr[s][1]; zq[s][0] = vq[s][0]; zq[s][1] = vq[s][1];
        ur[s][0] = fma(na1[s], u0r, fma(na2[s], u1r, xfr)); ur[s][1] = u0r;
        uq[s][0] = fma(na1[s], u0q, fma(na2[s], u1q, xfq)); uq[s][1] = u0q;
    }
    TDM_SCHED_FENCE();   // (the scans' table loads stay behind the segment totals' last use)
}

// the two bytes of sample k as one word (re in the low byte), and the integers in it
TDM_HD uint32_t pz_raw_pair(const void *rowp, int64_t k)
{
    const uint8_t *p = (const uint8_t *)rowp + 2 * k;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
}
template <int FMT8>
TDM_HD void pz_raw_unpair(uint32_t w, int &re, int &im)
{
    re = FMT8 == FMT_CU8 ? (int)(w & 0xffu) : (int)(int8_t)(w & 0xffu);
    im = FMT8 == FMT_CU8 ? (int)((w >> 8) & 0xffu) : (int)(int8_t)((w >> 8) & 0xffu);
}

// ------------------------------------------------------------------------------------------
// The edge slots of a wide block, built by the whole wavefront.  A wide block has at most kSlots lanes that hold samples of
// the odd extension or positions past the extended row (PzEdgeGeom): the first kHead lanes of block 0 and the kTail lanes
// from the one with the signal's last sample on, which may straddle two blocks.  Their kSlots * L int16 pairs are
// elements j = slot * L + i of Comm::edge_slots(); every lane takes the elements lane, lane + 64, ... (a fully unrolled share
// of ceil(kSlots L / 64)), reads the two anchors u[0] and u[n-1] once, issues the loads of all its elements, and writes its
// share in one pass.  The integers are those of the per-lane loop in pz_raw_body (2 u[0] - u[EDGE - e], the row's own
// samples, 2 u[n-1] - u[n-2-(e-EDGE-n)]; PzRawBias inside the extended row, true zero outside it).  An element outside
// the extended row, or of a slot whose lane belongs to another block, issues no load; the latter is not written either.
// The caller's wave_sync() stands between this and the edge lanes' reads.
// ------------------------------------------------------------------------------------------
template <int L, int EDGE, int FMT8, class Comm>
TDM_HD void pz_raw_fill_edges(Comm &cm, const char *rowp, int64_t n, int blk, int lane)
{
    typedef PzEdgeGeom<L, EDGE> G;
    constexpr int N = G::kSlots * L, PER = (N + kWave - 1) / kWave;
    const int64_t blk0 = (int64_t)blk * (kWave * L);
    const int64_t seg_t0 = ((G::P0 + EDGE + n) / L) * L;   // first position of the lane with the signal's last sample
    uint32_t *buf = (uint32_t *)cm.edge_slots();
    uint32_t wa0 = pz_raw_pair(rowp, 0), wa1 = pz_raw_pair(rowp, n - 1);
    uint32_t w[PER];
    bool mine[PER];
    int kind[PER];   // 0: outside the extended row, 1: head extension, 2: the row itself, 3: tail extension
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int j = lane + k * kWave;
        const int slot = j / L, i = j - slot * L;
        const int64_t seg = slot < G::kHead ? (int64_t)slot * L : seg_t0 + (int64_t)(slot - G::kHead) * L;
        const int64_t e = seg - G::P0 + i, d = e - EDGE;   // d: the position counted from the row's first sample
        mine[k] = j < N && seg >= blk0 && seg < blk0 + kWave * L;
        kind[k] = (!mine[k] || e < 0 || e >= n + 2 * (int64_t)EDGE) ? 0 : (d < 0 ? 1 : (d < n ? 2 : 3));
        // the sample read is the position mirrored at the row's end it lies beyond: EDGE - e, e - EDGE, n - 2 - (e - EDGE - n)
        w[k] = 0;
        if (kind[k]) w[k] = pz_raw_pair(rowp, d < 0 ? -d : (d < n ? d : 2 * (n - 1) - d));
    }
    // (every load above is in flight before the first of them is waited for: the words are first looked at from here on)
    TDM_OPAQUE_V(wa0);
    TDM_OPAQUE_V(wa1);
#pragma unroll
    for (int k = 0; k < PER; ++k) TDM_OPAQUE_V(w[k]);
    int a0r, a0i, a1r, a1i;
    pz_raw_unpair<FMT8>(wa0, a0r, a0i);
    pz_raw_unpair<FMT8>(wa1, a1r, a1i);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        int vr, vi;
        pz_raw_unpair<FMT8>(w[k], vr, vi);
        if (kind[k] == 1) { vr = 2 * a0r - vr; vi = 2 * a0i - vi; }
        if (kind[k] == 3) { vr = 2 * a1r - vr; vi = 2 * a1i - vi; }
        if (kind[k]) { vr += PzRawBias<FMT8>::value; vi += PzRawBias<FMT8>::value; }   // (2 (a + B) - (b + B) = 2 a - b + B)
        if (mine[k]) buf[lane + k * kWave] = kind[k] ? ((uint32_t)vr & 0xffffu) | ((uint32_t)vi << 16) : 0u;
    }
}

// PRUNE: the scans without the terms PzScanKeep<Q, S> leaves out (what ships); false: every term (tdm_debug_set
// "scan_prune" 0, and any plan whose design the compiled table does not fit)
template <int Q, int S, int EDGE, int FMT8, bool WIDE, bool FOLD = true, bool PRUNE = true, class Comm>
TDM_HD void pz_raw_body(const ZpParams &P, const void *iq, int64_t row_stride, Comm &cm, int lane, int blk, int row)
{
    constexpr int NP = PzLayout::kMaxPairs;
    constexpr int L = Q * S;
    constexpr int NR = WIDE ? L : L / 2;
    static_assert(L % 2 == 0, "two samples per dword");
    typedef PzEdgeGeom<L, EDGE> G;
    const int64_t n = P.n;
    const int64_t seg = (int64_t)blk * (kWave * L) + (int64_t)lane * L;
    const int64_t e0 = seg - G::P0;   // ext index of the lane's first sample
    const char *rowp = (const char *)iq + (int64_t)row * row_stride * 2;
    uint32_t raw[NR];
    if constexpr (WIDE) {
        // (a wavefront-uniform choice, made before the lanes part ways: every lane reaches the one wave_sync)
        if (!P.raw_edge_loop) {
            pz_raw_fill_edges<L, EDGE, FMT8>(cm, rowp, n, blk, lane);
            cm.wave_sync();
        }
    }
    if (e0 >= EDGE && e0 + L <= EDGE + n) {
        const char *p = rowp + (e0 - EDGE) * 2;
        uint32_t w[L / 2];
        if ((((uintptr_t)p) & 3) == 0) {
            const uint32_t *dw = (const uint32_t *)p;   // (4-byte aligned: merged into 16-byte loads)
#pragma unroll
            for (int c = 0; c < L / 2; ++c) w[c] = dw[c];
        } else {
            const uint16_t *h = (const uint16_t *)p;
#pragma unroll
            for (int c = 0; c < L / 2; ++c) w[c] = (uint32_t)h[2 * c] | ((uint32_t)h[2 * c + 1] << 16);
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            if (WIDE) {
                const uint32_t b = w[i / 2] >> (16 * (i % 2));
                const int re = (FMT8 == FMT_CU8 ? (int)(b & 0xffu) : (int)(int8_t)(b & 0xffu)) + PzRawBias<FMT8>::value;
                const int im = (FMT8 == FMT_CU8 ? (int)((b >> 8) & 0xffu) : (int)(int8_t)((b >> 8) & 0xffu)) + PzRawBias<FMT8>::value;
                raw[i] = ((uint32_t)re & 0xffffu) | ((uint32_t)im << 16);
            } else {
                raw[i] = w[i];
            }
        }
    } else if (!WIDE || e0 >= n + 2 * (int64_t)EDGE) {
        // (nothing of the extended row in this lane: zeros, WITHOUT the bias -- the constant the host removes is the one over
        //  the extended row.  A narrow block never comes here: it holds neither an extension sample nor a position outside
        //  the row, see the launch; its permute conversion could not make a zero)
#pragma unroll
        for (int c = 0; c < NR; ++c) raw[c] = 0;
    } else {
        int slot;
        if (e0 < EDGE) {
            slot = (int)(seg / L);
        } else {
            const int64_t seg_t0 = ((G::P0 + EDGE + n) / L) * L;
            slot = G::kHead + (int)((seg - seg_t0) / L);
        }
        uint32_t *buf = (uint32_t *)cm.edge_slots() + (size_t)slot * L;
        // ZpParams::raw_edge_loop (tdm_debug_set "raw_edge_fill" 0): the lane builds its slot itself, sample by sample --
        // what pz_raw_fill_edges replaced, kept as its A/B partner
        if (P.raw_edge_loop) {
#pragma unroll 1
            for (int i = 0; i < L; ++i) {
                const int64_t e = e0 + i;
                int re = 0, im = 0;
                if (e >= 0 && e < n + 2 * (int64_t)EDGE) {
                    if (e < EDGE) {  // 2*x[0] - x[edge - e]
                        int ar, ai;
                        pz_raw_sample<FMT8>(rowp, 0, ar, ai);
                        pz_raw_sample<FMT8>(rowp, EDGE - e, re, im);
                        re = 2 * ar - re;
                        im = 2 * ai - im;
                    } else if (e < EDGE + n) {
                        pz_raw_sample<FMT8>(rowp, e - EDGE, re, im);
                    } else {  // 2*x[n-1] - x[n-2-(e-edge-n)]
                        int ar, ai;
                        pz_raw_sample<FMT8>(rowp, n - 1, ar, ai);
                        pz_raw_sample<FMT8>(rowp, n - 2 - (e - EDGE - n), re, im);
                        re = 2 * ar - re;
                        im = 2 * ai - im;
                    }
                    re += PzRawBias<FMT8>::value;   // (2 (a + B) - (b + B) = 2 a - b + B: the extension of the biased row)
                    im += PzRawBias<FMT8>::value;
                }
                buf[i] = ((uint32_t)re & 0xffffu) | ((uint32_t)im << 16);
            }
        }
#pragma unroll
        for (int i = 0; i < NR; ++i) raw[i] = buf[i];
    }

    const auto pz = TDM_CPTR(P.pz);
    double yr[S], yi[S];
    double zr[NP][2], zq[NP][2], ur[NP][2], uq[NP][2];
    if constexpr (!WIDE && FOLD && PzRawFold<Q>::value) {
        pz_raw_fold_lane<Q, S, FMT8>(P, raw, cm.edge_slots() + lane, zr, zq, ur, uq, yr, yi);
    } else {
        const bool inject = (blk == 0 && lane == 0);
        // the four standing operand pairs of the conversions (pz_raw_perm): forward re / im, backward re / im
        double xfr, xfq, xbr, xbq;
        pz_raw_slot_init(xfr); pz_raw_slot_init(xfq); pz_raw_slot_init(xbr); pz_raw_slot_init(xbq);
        double e0r, e0i;
        pz_raw_cvt<FMT8, WIDE, true>(raw, G::P0, xfr, xfq);
        e0r = xfr; e0i = xfq;
        {
            const double dx = pz[PzLayout::off_dx];
#pragma unroll
            for (int t = 0; t < S; ++t) {
                pz_raw_cvt<FMT8, WIDE, true>(raw, t * Q, xbr, xbq);
                yr[t] = dx * xbr;
                yi[t] = dx * xbq;
            }
        }
        // ---------------- phase 1: all pole pairs per sample (a sample is converted once per direction) ----------------
        double na1[NP], na2[NP], b0[NP], b1[NP];
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            na1[s] = -pz[PzLayout::off_a1 + s];
            na2[s] = -pz[PzLayout::off_a2 + s];
            b0[s] = pz[PzLayout::off_b0 + s];
            b1[s] = pz[PzLayout::off_b1 + s];
        }
        double f1r[NP], f2r[NP], f1q[NP], f2q[NP], a1r[NP], a2r[NP], a1q[NP], a2q[NP];
#pragma unroll
        for (int s = 0; s < NP; ++s) { f1r[s] = 0; f2r[s] = 0; f1q[s] = 0; f2q[s] = 0; a1r[s] = 0; a2r[s] = 0; a1q[s] = 0; a2q[s] = 0; }
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const int ib = L - 1 - i;
            if (i == G::P0) {
                // scipy's zi*ext[0]: constant history ext[0] before the first extended sample
#pragma unroll
                for (int s = 0; s < NP; ++s) {
                    const double g = pz[PzLayout::off_g + s];
                    f1r[s] = inject ? g * e0r : f1r[s]; f2r[s] = inject ? g * e0r : f2r[s];
                    f1q[s] = inject ? g * e0i : f1q[s]; f2q[s] = inject ? g * e0i : f2q[s];
                }
            }
            pz_raw_cvt<FMT8, WIDE, true>(raw, i, xfr, xfq);
            pz_raw_cvt<FMT8, WIDE, true>(raw, ib, xbr, xbq);
#pragma unroll
            for (int s = 0; s < NP; ++s) {
                const double wr = fma(na1[s], f1r[s], fma(na2[s], f2r[s], xfr)), wq = fma(na1[s], f1q[s], fma(na2[s], f2q[s], xfq));
                if (i % Q == 0) {
                    yr[i / Q] = fma(b0[s], wr, fma(b1[s], f1r[s], yr[i / Q]));
                    yi[i / Q] = fma(b0[s], wq, fma(b1[s], f1q[s], yi[i / Q]));
                }
                f2r[s] = f1r[s]; f1r[s] = wr; f2q[s] = f1q[s]; f1q[s] = wq;
                const double vr = fma(na1[s], a1r[s], fma(na2[s], a2r[s], xbr)), vq = fma(na1[s], a1q[s], fma(na2[s], a2q[s], xbq));
                if (ib % Q == 0) {
                    yr[ib / Q] = fma(b0[s], vr, fma(b1[s], a1r[s], yr[ib / Q]));
                    yi[ib / Q] = fma(b0[s], vq, fma(b1[s], a1q[s], yi[ib / Q]));
                }
                a2r[s] = a1r[s]; a1r[s] = vr; a2q[s] = a1q[s]; a1q[s] = vq;
            }
            // one sample step at a time (see TDM_PIN): keeps conversions and chains of later steps from being hoisted
#pragma unroll
            for (int s = 0; s < NP; ++s) { TDM_PIN(f1r[s]); TDM_PIN(f1q[s]); TDM_PIN(a1r[s]); TDM_PIN(a1q[s]); }
            if (i % Q == 0) { TDM_PIN(yr[i / Q]); TDM_PIN(yi[i / Q]); }
            if (ib % Q == 0) { TDM_PIN(yr[ib / Q]); TDM_PIN(yi[ib / Q]); }
        }
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            zr[s][0] = f1r[s]; zr[s][1] = f2r[s]; zq[s][0] = f1q[s]; zq[s][1] = f2q[s];
            ur[s][0] = a1r[s]; ur[s][1] = a2r[s]; uq[s][0] = a1q[s]; uq[s][1] = a2q[s];
        }
    }
    typedef std::conditional_t<PRUNE, PzScanKeep<Q, S>, PzScanKeepAll> Keep;
    pz_block_finish<Q, S, EDGE, Keep, true>(P, cm, lane, blk, row, zr, zq, ur, uq, yr, yi, pz[PzLayout::off_yc]);
    // the last extended sample, as an integer: 2 u[n-1] - u[n-1-edge]
    if (blk == P.nb - 1 && lane == 0) {
        int ar, ai, br, bi;
        pz_raw_sample<FMT8>(rowp, n - 1, ar, ai);
        pz_raw_sample<FMT8>(rowp, n - 1 - EDGE, br, bi);
        P.flast[(int64_t)row * 2] = (double)(2 * ar - br + PzRawBias<FMT8>::value);
        P.flast[(int64_t)row * 2 + 1] = (double)(2 * ai - bi + PzRawBias<FMT8>::value);
    }
}

// Start of the anticausal carry chain (scipy: backward pass started at zi * forward output at the last
// sample).  G = resolved causal carry into the last block, El = exported lane state, xl = ext[last].
template <int D>
TDM_HD void pz_carry_last(const ZpParams &P, int row, int ch, const double *G)
{
    const int nb = P.nb;
    const int S = P.L / P.out_stride;
    const auto AG = TDM_CPTR(P.pz + PzLayout::off_AG(S));
    const auto AE = TDM_CPTR(P.pz + PzLayout::off_AE(S));
    const auto wx = TDM_CPTR(P.pz + PzLayout::off_wx(S));
    const double *El = P.Elast + (int64_t)row * D * 2 + ch;
    const double xl = P.flast[(int64_t)row * 2 + ch];
    double *Hb = P.Hb + (int64_t)row * nb * D * 2 + ch;
    double e[D];
#pragma unroll
    for (int k = 0; k < D; ++k) e[k] = El[k * 2];
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double acc = wx[r] * xl;
#pragma unroll
        for (int k = 0; k < D; ++k) acc += AG[r * D + k] * G[k] + AE[r * D + k] * e[k];
        Hb[((int64_t)(nb - 1) * D + r) * 2] = acc;
    }
}

// Both carries of a parallel-form stage in ONE pass (the two banks do not couple, so the anticausal carry of a block
// needs no other block's causal carry -- except through the start state at the end of the row, which the few
// threads near the end recompute for themselves).  Transitions are block-diagonal: 2x2 per pole pair.
//     Gf[b] = Mf Gf[b-1] + Ef[b-1],   Hb[b-1] = Mb(b) Hb[b] + Eb[b],   Hb[nb-1] from pz_carry_last's formula
// each evaluated as the Horner form of its series over P.carry_terms blocks (see zp_carry_fwd_body).
// which = 0: the causal carry Gf[b] into block b, which = 1: the anticausal carry Hb[b]; component ch (0 re, 1 im) -> out[D].
// Self-contained (reads only the block-local end states the decimator kernel wrote), so the low-rate kernel's carry-
// response items can form the carry they need themselves and the separate carry launch falls away (lp2_kernels.hpp).
// SCALAR_END: the three D x D matrices of the row-end formula through scalar loads (the carry kernel: every thread of a
// launch may need them) or through ordinary loads inside the branch (the low-rate kernel's items: one item in hundreds
// takes that branch, and 192 scalar registers of hoisted loads spill)
template <int NSEC, bool SCALAR_END = true>
TDM_HD void pz_carry_compute(const ZpParams &P, int row, int b, int ch, int which, double *out)
{
    constexpr int D = 2 * NSEC;
    const int nb = P.nb, terms = P.carry_terms;
    const int64_t base = (int64_t)row * nb * D * 2 + ch;
    const double *Ef = P.Ef + base, *Eb = P.Eb + base;
    auto step_m = [&](const auto M, double *v, const double *e) {   // v <- M v + e, M block-diagonal
#pragma unroll
        for (int s = 0; s < NSEC; ++s) {
            const double a = v[2 * s], c = v[2 * s + 1];
            v[2 * s] = fma(M[(2 * s) * D + 2 * s], a, fma(M[(2 * s) * D + 2 * s + 1], c, e[(2 * s) * 2]));
            v[2 * s + 1] = fma(M[(2 * s + 1) * D + 2 * s], a, fma(M[(2 * s + 1) * D + 2 * s + 1], c, e[(2 * s + 1) * 2]));
        }
    };
    // (last: the transition over the shorter last block)
    auto step = [&](bool last, double *v, const double *e) {
        if (SCALAR_END) {
            if (last) step_m(TDM_CPTR(P.Mb_last), v, e);
            else step_m(TDM_CPTR(P.Mf), v, e);
        } else {
            step_m(last ? P.Mb_last : P.Mf, v, e);
        }
    };
    auto causal_carry = [&](int blk, double *G) {
#pragma unroll
        for (int k = 0; k < D; ++k) G[k] = 0;
        for (int bb = blk - terms > 0 ? blk - terms : 0; bb < blk; ++bb) step(false, G, Ef + (int64_t)bb * D * 2);
    };
    auto row_end_start = [&](const double *G, double *H) {   // pz_carry_last's formula
        const int S = P.L / P.out_stride;
        const double *El = P.Elast + (int64_t)row * D * 2 + ch;
        const double xl = P.flast[(int64_t)row * 2 + ch];
        auto apply = [&](const auto AG, const auto AE, const auto wx) {
#pragma unroll
            for (int r = 0; r < D; ++r) {
                double acc = wx[r] * xl;
#pragma unroll
                for (int k = 0; k < D; ++k) acc += AG[r * D + k] * G[k] + AE[r * D + k] * El[k * 2];
                H[r] = acc;
            }
        };
        if (SCALAR_END) apply(TDM_CPTR(P.pz + PzLayout::off_AG(S)), TDM_CPTR(P.pz + PzLayout::off_AE(S)), TDM_CPTR(P.pz + PzLayout::off_wx(S)));
        else apply(P.pz + PzLayout::off_AG(S), P.pz + PzLayout::off_AE(S), P.pz + PzLayout::off_wx(S));
    };
    if (which == 0) {
        causal_carry(b, out);
        return;
    }
    double *H = out;
    if (b == nb - 1) {
        double G[D];
        causal_carry(b, G);
        row_end_start(G, H);
    } else {
        int far = b + terms;
        if (far >= nb - 1) {
            far = nb - 1;
            double Gl[D];
            causal_carry(nb - 1, Gl);
            row_end_start(Gl, H);
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) H[k] = 0;
        }
        for (int bb = far; bb > b; --bb) step(bb == nb - 1, H, Eb + (int64_t)bb * D * 2);
    }
}

template <int NSEC>
TDM_HD void pz_carry_body(const ZpParams &P, int row, int b, int ch)
{
    constexpr int D = 2 * NSEC;
    const int64_t base = (int64_t)row * P.nb * D * 2 + ch;
    double G[D], H[D];
    pz_carry_compute<NSEC>(P, row, b, ch, 0, G);
#pragma unroll
    for (int k = 0; k < D; ++k) P.Gf[base + ((int64_t)b * D + k) * 2] = G[k];
    pz_carry_compute<NSEC>(P, row, b, ch, 1, H);
#pragma unroll
    for (int k = 0; k < D; ++k) P.Hb[base + ((int64_t)b * D + k) * 2] = H[k];
}

}  // namespace tdm
