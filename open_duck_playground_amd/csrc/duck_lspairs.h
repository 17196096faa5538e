// duck_lspairs.h — the line search's row-activity flag (duck_team.h quad2, quad2_pair).
//
// A one-sided row is active at alpha where x = ja + alpha v < 0, and its quadratic coefficients enter the
// point's (q0, q1, q2) through a 0/1 factor. As compare and select that factor is two instructions; as one
// saturating multiply, x times -2^127 clamped to [0, 1], it is one:
//   x < 0, normal (|x| >= 2^-126)  the product is >= 2, clamped to 1       -inf -> +inf -> 1
//   x > 0                          the product is negative, clamped to 0   +inf -> -inf -> 0
//   x = +-0                        -+0, clamped to +0
//   x = NaN                        NaN, which the clamp turns into 0 (the kernels run with DX10_CLAMP on),
//                                  as NaN < 0 is false
//   x denormal                     the multiply reads 0 (the kernels flush denormals), as the compare does
// tests/test_gpu_ls_pairs.py feeds both forms these classes on the GPU (duck_debug_ls_flag) and asserts
// equal words. -DDUCK_SCALAR_TWINS (the test build of the scalar line search): compare and select.
// Both halves of a pair in one v_pk_mul_f32 ... clamp was measured and not kept: the compiler has no packed
// form of the clamp (a packed multiply and min / max compile to the multiply and a clamping v_max_f32 per
// half), and the instruction written by name gave the same words but, in the flat step kernel, took 4
// v_readlane and 3 wait states for the 4 slots it saved (profiles/r13_packed_ab.txt).
#pragma once
#include "duck_math.h"

typedef float f2v __attribute__((ext_vector_type(2)));

DK float ls_flag_select(float x) { return x < 0.0f ? 1.0f : 0.0f; }
// (the median of three with 0 and 1 compiles to the multiply's clamp modifier: v_mul_f32 ... clamp)
DK float ls_flag_sat(float x) { return __builtin_amdgcn_fmed3f(x * -0x1p127f, 0.0f, 1.0f); }
template <bool SAT>
DK float ls_flag(float x) {
  return SAT ? ls_flag_sat(x) : ls_flag_select(x);
}

// The scenes whose line search takes the saturating flag and, in the throughput kernel, the paired bracket
// ends (duck_team.h quad2_pair): all but a height-field scene without backlash. Measured, alternating runs
// against the parent on one box (profiles/r13_packed_ab.txt): flat C2 +1.0 %, C3 +1.5 %, rough + backlash
// C5 +0.3 % (above the parent's interval), rough C4 -0.2 % in kernel time, below the parent's interval: its
// line search shrinks as flat's does (region 13: 390 -> 338 instructions), but the registers around it come
// out differently (ten more v_readlane / v_writelane per substep in the solves, 38 wait states more in the
// sensors), so that scene keeps the parent's code. The condition is a proxy (a height field and at most 16
// limit rows), not a measured property of a model; neither form moves a bit, only time.
// -DDUCK_SCALAR_TWINS: no scene.
template <class Md>
constexpr bool ls_pairs() {
#ifdef DUCK_SCALAR_TWINS
  return false;
#else
  return !(Md::FLOOR_TYPE == 1 && Md::NLIM <= 16);
#endif
}

// The scenes whose fused warm start (duck_team.h warm_start: the throughput kernel and physics_kernel) runs
// its two starts' chains, qacc_warmstart and qacc_smooth, as packed pairs (warm_rows_pair, spatial2_pair).
// Neither form moves a bit; a scene whose measured interval falls below its parent's keeps the scalar form
// (warm_rows_both's own statements). Every scene takes the pairs: against the scalar form with the same
// stores, C2 23.07-23.12 for 22.93-22.96 M env-steps/s (profiles/r15_warm_pairs_ab.txt, section 1).
// -DDUCK_SCALAR_TWINS (the scalar_twins test library of __graft_entry__.build()): no scene.
// -DDUCK_SCALAR_WARM: no scene either, beside the paired line search; the library of that A/B, built by hand as
// native.build(defines=["DUCK_SCALAR_WARM"], out=".../libduck_sw.so") and timed with tools/gpu_ab_libs.sh.
template <class Md>
constexpr bool warm_pairs() {
#if defined(DUCK_SCALAR_TWINS) || defined(DUCK_SCALAR_WARM)
  return false;
#else
  return true;
#endif
}
