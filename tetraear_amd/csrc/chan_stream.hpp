// Position arithmetic of the stateful channeliser (include/tetrahip.h tdm_channeliser_*): host and device, no HIP, so that a
// CPU test can compile it alone with g++ and hold it to a Python statement of the same rule.
//
// A stream's samples are counted from its start (absolute index a); output m_abs sits at input instant a = m_abs*D
// (oracle/pfb_np.py, x[a] = 0 for a < 0).  A push hands over n samples a = pos .. pos+n-1 as local indices 0 .. n-1 and
// emits every output whose instant falls among them:
//     n_out  = ceil((pos+n)/D) - ceil(pos/D)        (may be 0)
//     o      = ceil(pos/D)*D - pos                  local index of the first instant, in [0, D)
//     s_base = (ceil(pos/D)*D) mod M                the first output's phase shift (stage A's circular shift)
// Local output m then reads the window o + m*D - (L-1) .. o + m*D.  Local indices n < 0 come from the history, the last
// L-1 samples before the push (history slot j holds local index j - (L-1)); only the last `hist_valid` = min(pos, L-1) of
// them exist -- the samples before the stream's start read as zero through that count, not through stored bytes (a cu8 byte
// cannot encode 0.0).  The next history is the last L-1 of (old history || this push): slot j takes local index
// n - (L-1) + j, from the push when that is >= 0, else from old slot j + n.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TDM_CS_HD __host__ __device__
#else
#define TDM_CS_HD
#endif

namespace tdm {

TDM_CS_HD inline int64_t cs_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }   // a >= 0, b >= 1

struct ChanPush {
    int64_t n_out;        // outputs of this push
    int64_t o;            // local input index of the first output instant, [0, D)
    int32_t s_base;       // (first output's absolute instant) mod M
    int32_t hist_valid;   // history samples that precede this push and belong to the stream, [0, L-1]
};

// pos: samples the stream had before this push; n >= 0 samples in it
TDM_CS_HD inline ChanPush chan_push(int64_t pos, int64_t n, int32_t M, int32_t D, int32_t L)
{
    ChanPush p;
    const int64_t m_abs = cs_ceil_div(pos, D);   // outputs before this push = index of its first output
    p.n_out = cs_ceil_div(pos + n, D) - m_abs;
    p.o = m_abs * D - pos;
    p.s_base = (int32_t)(((m_abs % M) * (int64_t)(D % M)) % M);   // no overflow for any int64 position
    p.hist_valid = (int32_t)(pos < L - 1 ? pos : L - 1);
    return p;
}

// where slot j of the NEXT history comes from after a push of n samples: >= 0 a local index of the push, < 0 slot
// (-1 - value) of the old history
TDM_CS_HD inline int64_t chan_hist_source(int64_t j, int64_t n, int32_t L)
{
    const int64_t src = n - (L - 1) + j;
    return src >= 0 ? src : -1 - (j + n);
}

}  // namespace tdm
