// TEST INFRASTRUCTURE ONLY -- the emulated cu8 chain with the raw-integer decimator's lane scans in EITHER form, and the
// compiled table of kept scan terms beside the design it was made for (tests/test_scan_prune_cpu.py).  emul.cpp reaches
// only the shipped form of pz_raw_body (PRUNE = true: the scans without the terms PzScanKeep leaves out); this harness
// also instantiates the same body with every term.  Compiled by the test with g++ into its own shared object; never part
// of the product.
#include "emul.cpp"

namespace {

struct EmuBackendAllTerms : EmuBackend {
    template <int Q, int S, int EDGE, int FMT8>
    void pz_raw(const ZpParams &P, const void *iq, int64_t stride, int b_tail, int rows)
    {
        for (int row = 0; row < rows; ++row)
            for (int blk = 0; blk < P.nb; ++blk)
                run_group(kWave, [&](int lane, Group *g) {
                    EmuWaveComm cm{g, lane};
                    if (blk == 0 || blk >= b_tail)
                        pz_raw_body<Q, S, EDGE, FMT8, true, true, false>(P, iq, stride, cm, lane, blk, row);
                    else
                        pz_raw_body<Q, S, EDGE, FMT8, false, true, false>(P, iq, stride, cm, lane, blk, row);
                });
    }
};

// Mirrors emu_process() of emul.cpp (plan, buffer binding, run_ref) for cu8 rows on the raw-integer path; a change to the
// set-up there has to be repeated here.
template <class BE>
int run_rows(double sample_rate, int64_t n, int rows, const void *iq, int64_t stride, const double *freq_offset, uint8_t *hard,
             double *soft, int32_t *n_soft, int32_t *best_phase, int32_t *max_soft_out)
{
    RefPlanHost h = build_ref_plan(sample_rate, n, 25000.0, true, FMT_CU8);
    if (max_soft_out) *max_soft_out = (int32_t)h.max_soft;
    if (!h.lp2.ok || !h.raw_S) return -1;   // (this length / rate does not take the raw-integer decimator)
    if (!iq) return 0;
    HostZp dec, dec_raw;
    RefBuffers B;
    dec.t = h.dec; dec.bind(rows); B.dec_params = dec.t.p;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> zt, lp2p;
    B.lp2 = h.lp2.p;
    zt.assign((size_t)rows * h.sps * B.lp2.zt_k * 2 + 2, nan);
    B.lp2.zt = zt.data();
    B.lp2.lane_m = h.lp2.lane_m.data();
    B.lp2.cst = h.lp2.cst.data();
    B.lp2.seeds = h.lp2.seeds.data();
    B.lp2.items = (const int32_t *)h.lp2.items.data();
    dec_raw.t = h.dec_raw;
    dec_raw.bind(rows);
    B.dec_raw_params = dec_raw.t.p;
    B.lp2_raw = h.lp2_raw.p;
    lp2p.assign((size_t)rows * std::max(B.lp2_raw.n_chunks, B.lp2.n_chunks) * kMaxSps + 2, nan);
    B.lp2.partials = lp2p.data();
    B.lp2_raw.zt = zt.data();
    B.lp2_raw.partials = lp2p.data();
    B.lp2_raw.lane_m = h.lp2.lane_m.data();
    B.lp2_raw.cst = h.lp2_raw.cst.data();
    B.lp2_raw.seeds = h.lp2_raw.seeds.data();
    B.lp2_raw.items = (const int32_t *)h.lp2_raw.items.data();
    std::vector<double> y((size_t)rows * h.n_dec * 2 + 2, nan), z((size_t)rows * h.n_dec * 2 + 2, nan);
    B.y = y.data();
    B.z = z.data();
    std::vector<double> partials((size_t)rows * (h.n_dec / kPowThreads + 16) * kMaxSps, nan);
    B.partials = partials.data();
    std::vector<double> mm((size_t)rows, 0.0);
    RefIO io{iq, stride, nullptr, freq_offset, hard, soft, n_soft, best_phase, mm.data(), 0, 1};
    BE be;
    run_ref(be, h, rows, FMT_CU8, B, io);
    return 0;
}

}  // namespace

extern "C" {

// prune != 0: the shipped form of the lane scans; 0: every term.  iq == null: sizes only.
// returns 0, or -1 when the plan of this rate and length does not take the raw-integer decimator
int spr_run(int prune, double sample_rate, int64_t n, int rows, const void *iq, int64_t stride, const double *freq_offset,
            uint8_t *hard, double *soft, int32_t *n_soft, int32_t *best_phase, int32_t *max_soft)
{
    if (prune) return run_rows<EmuBackend>(sample_rate, n, rows, iq, stride, freq_offset, hard, soft, n_soft, best_phase, max_soft);
    return run_rows<EmuBackendAllTerms>(sample_rate, n, rows, iq, stride, freq_offset, hard, soft, n_soft, best_phase, max_soft);
}

// The compiled table of the factor this sample rate decimates by, beside the plan's own design, pairs in the ORDER OF THE
// TABLES the kernel indexes (PzShared::dz: the order of Mpow and of the lane tables):
//   geom = {q, S, L, terms};  kept[4];  a2[4] = |pole|^2 of each pair as the tables hold it;
//   below[4][terms] = 1 where the long-double bound |p|^(L 2^term) is under the constant;  bound[4][terms] = the bound
//   rounded to double (for messages);  *constant = the constant;  *plan_ok = what the plan's own check said
// returns 0, or -1 when no raw-integer kernel exists for the rate
int spr_table(double sample_rate, int32_t *geom, int32_t *kept, double *a2, int32_t *below, double *bound, double *constant,
              int32_t *plan_ok)
{
    RefPlanHost h = build_ref_plan(sample_rate, 100000, 25000.0, true, FMT_CU8);
    if (!h.raw_S || !h.dec_raw.shared) return -1;
    const PzShared &sh = *std::static_pointer_cast<const PzShared>(h.dec_raw.shared);
    geom[0] = h.q; geom[1] = h.raw_S; geom[2] = sh.L; geom[3] = kPzScanTerms;
    for (int s = 0; s < PzLayout::kMaxPairs; ++s) {
        kept[s] = pz_raw_scan_kept(h.q, s);
        a2[s] = (double)sh.dz.a2[s];
        for (int t = 0; t < kPzScanTerms; ++t) {
            const long double b = pz_scan_bound(sh.dz, s, sh.L, t);
            below[s * kPzScanTerms + t] = b < kPzScanNegligible ? 1 : 0;
            bound[s * kPzScanTerms + t] = (double)b;
        }
    }
    *constant = (double)kPzScanNegligible;
    *plan_ok = h.raw_scan_prune_ok ? 1 : 0;
    return 0;
}

// pz_scan_keep_is_safe on the plan's design with a table of the caller's (the check tdm_plan_create relies on)
int spr_table_is_safe(double sample_rate, const int32_t *kept)
{
    RefPlanHost h = build_ref_plan(sample_rate, 100000, 25000.0, true, FMT_CU8);
    if (!h.raw_S || !h.dec_raw.shared) return -1;
    const PzShared &sh = *std::static_pointer_cast<const PzShared>(h.dec_raw.shared);
    int k[PzLayout::kMaxPairs];
    for (int s = 0; s < PzLayout::kMaxPairs; ++s) k[s] = kept[s];
    return pz_scan_keep_is_safe(sh.dz, sh.L, k) ? 1 : 0;
}
}
