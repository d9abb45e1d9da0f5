// TEST INFRASTRUCTURE ONLY -- the emulated cu8 chain with the raw-integer decimator's narrow blocks in EITHER form
// (tests/test_pz_fold_cpu.py).  emul.cpp reaches only the shipped form of pz_raw_body (the folded block sums at q = 10);
// this harness also instantiates the per-sample form of the same body, and hands out the decimator's finished output
// (block-local part + carry responses) next to the symbols, so that both forms can be held against the oracle.
// Compiled by the test with g++ into its own shared object; never part of the product.
#include "emul.cpp"

namespace {

struct EmuBackendPerSample : EmuBackend {
    template <int Q, int S, int EDGE, int FMT8>
    void pz_raw(const ZpParams &P, const void *iq, int64_t stride, int b_tail, int rows)
    {
        for (int row = 0; row < rows; ++row)
            for (int blk = 0; blk < P.nb; ++blk)
                run_group(kWave, [&](int lane, Group *g) {
                    EmuWaveComm cm{g, lane};
                    if (blk == 0 || blk >= b_tail)
                        pz_raw_body<Q, S, EDGE, FMT8, true, false>(P, iq, stride, cm, lane, blk, row);
                    else
                        pz_raw_body<Q, S, EDGE, FMT8, false, false>(P, iq, stride, cm, lane, blk, row);
                });
    }
};

// Mirrors emu_process() of emul.cpp (plan, buffer binding, run_ref) for one cu8 row on the raw-integer path; a change to
// the set-up there has to be repeated here.
template <class BE>
int run_one(double sample_rate, int64_t n, const void *iq, double freq_offset, double *y_dec, uint8_t *hard, double *soft,
            int32_t *n_soft, int32_t *best_phase, int64_t *n_dec_out, int32_t *max_soft_out, int32_t *narrow_blocks)
{
    const int rows = 1;
    RefPlanHost h = build_ref_plan(sample_rate, n, 25000.0, true, FMT_CU8);
    if (n_dec_out) *n_dec_out = h.n_dec;
    if (max_soft_out) *max_soft_out = (int32_t)h.max_soft;
    if (!h.lp2.ok || !h.raw_S) return -1;   // (this length / rate does not take the raw-integer decimator)
    {
        const ZpParams &p = h.dec_raw.p;
        if (narrow_blocks) *narrow_blocks = pz_raw_first_tail_block(p) - 1;
    }
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
    double mm = 0;
    RefIO io{iq, n, nullptr, &freq_offset, hard, soft, n_soft, best_phase, &mm, 0, 1};
    BE be;
    run_ref(be, h, rows, FMT_CU8, B, io);
    // the decimator's finished output, without the frequency shift the low-rate stage applies on load
    be.template zp_fixup<8, kLDec>(B.dec_raw_params, B.dec_raw_params.nb, rows, y_dec, h.n_dec, nullptr, h.rate_dec);
    return 0;
}

}  // namespace

extern "C" {

// fold != 0: the shipped form of the narrow blocks; 0: the per-sample form.  iq == null: sizes only.
// returns 0, or -1 when the plan of this rate and length does not take the raw-integer decimator
int pzf_run(int fold, double sample_rate, int64_t n, const void *iq, double freq_offset, double *y_dec, uint8_t *hard,
            double *soft, int32_t *n_soft, int32_t *best_phase, int64_t *n_dec, int32_t *max_soft, int32_t *narrow_blocks)
{
    if (fold)
        return run_one<EmuBackend>(sample_rate, n, iq, freq_offset, y_dec, hard, soft, n_soft, best_phase, n_dec, max_soft, narrow_blocks);
    return run_one<EmuBackendPerSample>(sample_rate, n, iq, freq_offset, y_dec, hard, soft, n_soft, best_phase, n_dec, max_soft, narrow_blocks);
}
}
