// The IQ wire formats, defined once: codes, sizes, decodes, the run-time -> compile-time dispatch and which entry point takes
// which.  Kernels, host code and (through tests/emul, compiled by g++) the CPU tests read this file; Python's table is
// tetraear_amd/_lib.py WIRE_FORMATS.  Plain scalar types only: a site that works on a vector type wraps the scalars here.
//   cu8   uint8 I, Q    value = u * fl(1/127.5) - 1   (pyrtlsdr: numpy's complex / real division multiplies by the rounded
//                                                      reciprocal -- two roundings in fp64, never one fma)
//   cs8   int8 I, Q     value = s / 128               (exact)
//   cs16  int16 I, Q    value = s / 32768             (exact; one 4-byte word per sample, I in the low half)
//   cf32 / cf64         the value itself
#pragma once
#include <stdint.h>
#include <type_traits>

#include "zp_common.hpp"

namespace tdm {

enum { FMT_CU8 = 0, FMT_CS8 = 1, FMT_CF32 = 2, FMT_CF64 = 3, FMT_CS16 = 4, FMT_COUNT = 5 };   // include/tetrahip.h TDM_CU8 ...

// bytes per complex sample.  (fmt by reference: where a kernel passes a field of its arguments, every comparison reads that
// field as the chain it used to spell out did -- by value the compiler folds the chain into selects, which moves k_gate's and
// k_pz_block's registers)
TDM_HD constexpr int wire_bytes(const int &fmt)
{
    return (fmt == FMT_CU8 || fmt == FMT_CS8) ? 2 : (fmt == FMT_CS16 ? 4 : (fmt == FMT_CF32 ? 8 : 16));
}
// the same for a consumer that never sees cf64 (kWireChan), as the shorter chain k_pfb was compiled with: that kernel takes
// its format at run time, and the five-way chain above costs it two instructions
constexpr int wire_bytes_fp32(int fmt) { return fmt == FMT_CF32 ? 8 : (fmt == FMT_CS16 ? 4 : 2); }
constexpr bool wire_packed8(int fmt) { return fmt == FMT_CU8 || fmt == FMT_CS8; }    // integer codes, 2 bytes per sample
constexpr bool wire_packed(int fmt) { return wire_packed8(fmt) || fmt == FMT_CS16; }  // integer codes: decoded where a kernel stages them

// ---- which entry point takes which format
constexpr unsigned wire_bit(int fmt) { return 1u << fmt; }
constexpr unsigned kWireAll = (1u << FMT_COUNT) - 1u;
constexpr unsigned kWireRefPlan = kWireAll, kWireGate = kWireAll;   // reference-mode plans, tdm_spectrum_gate
constexpr unsigned kWireTetra = kWireAll & ~wire_bit(FMT_CF64);     // TETRA-mode plans: fp32 kernels
constexpr unsigned kWireChan = kWireAll & ~wire_bit(FMT_CF64);      // the channeliser: fp32 kernels
// the host-fed stream: its page-locked slots and their numpy views were written before cs16 existed and nothing feeds them
// int16 pairs yet -- a feature that has not been built, not an ordering of the codes
constexpr unsigned kWireStream = kWireAll & ~wire_bit(FMT_CS16);
constexpr bool wire_accepts(unsigned mask, int fmt) { return fmt >= 0 && fmt < FMT_COUNT && ((mask >> fmt) & 1u); }
static_assert(wire_bytes_fp32(FMT_CU8) == wire_bytes(FMT_CU8) && wire_bytes_fp32(FMT_CS8) == wire_bytes(FMT_CS8) &&
              wire_bytes_fp32(FMT_CF32) == wire_bytes(FMT_CF32) && wire_bytes_fp32(FMT_CS16) == wire_bytes(FMT_CS16) &&
              !wire_accepts(kWireChan, FMT_CF64), "wire_bytes_fp32 is wire_bytes on the channeliser's formats");

// ---- run-time code -> compile-time constant: f(std::integral_constant<int, FMT>{}) for the format `fmt` names; a code
// outside MASK (or no code at all) goes to ELSE, which is what every caller's hand-written chain did with its default.  A
// kernel writes its f as [&](auto F) TDM_WIRE_INLINE { ... }: inlined before anything is optimised, the compiler sees the
// switch the kernel used to spell out.
#define TDM_WIRE_INLINE __attribute__((always_inline))
template <int FMT>
using WireFmt = std::integral_constant<int, FMT>;
template <unsigned MASK = kWireAll, int ELSE = FMT_CF64, class F>
TDM_HD auto wire_dispatch(int fmt, F &&f)
{
#define TDM_WIRE_CASE(X) \
    case X:              \
        if constexpr (((MASK >> X) & 1u) && X != ELSE) return f(WireFmt<X>{}); else break;
    switch (fmt) {
        TDM_WIRE_CASE(FMT_CU8) TDM_WIRE_CASE(FMT_CS8) TDM_WIRE_CASE(FMT_CF32) TDM_WIRE_CASE(FMT_CS16) TDM_WIRE_CASE(FMT_CF64)
    default: break;
    }
#undef TDM_WIRE_CASE
    return f(WireFmt<ELSE>{});
}

// ---- decode.  (HIP's __dmul_rn / __dsub_rn are plain operators and get contracted into one v_fma_f64 with a neighbouring
// operation under the default -ffp-contract=fast-honor-pragmas; the pragma is what keeps the two roundings)
TDM_HD double mul_rn(double a, double b)
{
#pragma clang fp contract(off)
    return a * b;
}
TDM_HD double add_rn(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}
TDM_HD double sub_rn(double a, double b)
{
#pragma clang fp contract(off)
    return a - b;
}

template <int FMT>
struct WireScale {   // value = code * scale, - 1 where biased
    static_assert(wire_packed(FMT), "cf32 / cf64 carry values, not codes");
    static constexpr bool biased = FMT == FMT_CU8;
    typedef std::conditional_t<FMT == FMT_CU8, uint8_t, std::conditional_t<FMT == FMT_CS8, int8_t, int16_t>> code;   // a component in memory
    static constexpr double f64 = FMT == FMT_CU8 ? 1.0 / 127.5 : (FMT == FMT_CS8 ? 1.0 / 128.0 : 0x1p-15);
    static constexpr float f32 = FMT == FMT_CU8 ? 1.f / 127.5f : (FMT == FMT_CS8 ? 1.f / 128.f : 0x1p-15f);
};

// the component codes of a packed sample: w holds it in its low 16 bits (cu8, cs8: I in the low byte) or is the whole word
// (cs16: I in the low half).  Each comes back in the integer type it was extracted as, so that the conversion to floating
// point that follows is the one instruction the hardware has for that field.
template <int FMT>
TDM_HD auto wire_code_i(uint32_t w)
{
    if constexpr (FMT == FMT_CU8) return w & 255u;
    else if constexpr (FMT == FMT_CS8) return (int8_t)(w & 255u);
    else return (int16_t)(w & 65535u);
}
template <int FMT>
TDM_HD auto wire_code_q(uint32_t w)
{
    if constexpr (FMT == FMT_CU8) return (w >> 8) & 255u;
    else if constexpr (FMT == FMT_CS8) return (int8_t)((w >> 8) & 255u);
    else return (int32_t)w >> 16;
}

// one component from its code (any integer type that holds it): fp64, and the same expression in fp32.  A device compiler
// may contract the fp32 cu8 multiply and subtract into one fma, which changes the low bit in 158 of the 256 codes: the fp32
// consumers are defined by their own oracles to that tolerance, and each keeps the form it was validated with.
template <int FMT, class C>
TDM_HD double wire_f64(C code)
{
    if (WireScale<FMT>::biased) return sub_rn(mul_rn((double)code, WireScale<FMT>::f64), 1.0);
    return (double)code * WireScale<FMT>::f64;
}
template <int FMT, class C>
TDM_HD float wire_f32(C code)
{
    if (WireScale<FMT>::biased) return (float)code * WireScale<FMT>::f32 - 1.f;
    return (float)code * WireScale<FMT>::f32;
}
// a sample from its packed word
template <int FMT>
TDM_HD void wire_f64(uint32_t w, double &re, double &im)
{
    re = wire_f64<FMT>(wire_code_i<FMT>(w));
    im = wire_f64<FMT>(wire_code_q<FMT>(w));
}
// the 8-bit formats from their two fields as unsigned bytes (the sign applied at the conversion), both extracted before either
// is converted: the order RawLoaderRT::fast8 (pz_kernels.hpp) was compiled with -- the word form gives k_pz_block another
// register allocation
template <int FMT>
TDM_HD void wire_f64_bytes(uint32_t bi, uint32_t bq, double &re, double &im)
{
    static_assert(wire_packed8(FMT), "two bytes per sample");
    if (FMT == FMT_CU8) {
        re = wire_f64<FMT>(bi);
        im = wire_f64<FMT>(bq);
    } else {
        re = wire_f64<FMT>((int8_t)bi);
        im = wire_f64<FMT>((int8_t)bq);
    }
}

}  // namespace tdm
