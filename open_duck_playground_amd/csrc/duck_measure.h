// duck_measure.h — everything of the env kernels that exists only in measurement, debug and test
// builds (native.debug_library): stage cycle counters, event counters, stage doubling, assembly
// marks, latency-kernel event times, the line search's dumps. The kernels call the macros below at
// fixed points; in the default build each of them expands to nothing (`do {} while (0)` where a
// statement is needed), and the constexpr switches are false.
//
//   -DDUCK_STAGE_PROF  per-stage cycle counters and event counters (tools/stage_prof.py)
//   -DDUCK_WAVE_PROF   only the per-wave launch cycles (no stage marks perturbing wave 0)
//   -DDUCK_LAT_PROF    latency kernels: stage cycles and event times of workgroup 0 (tools/lat_prof.py)
//   -DDUCK_ASM_MARKS   a comment at each stage boundary, no code (tools/isa_stage_hist.py)
//   -DDUCK_DOUBLE=k    stage k runs twice (tools/stage_pmc_summary.py; the list of k is below)
//   -DDUCK_LS_DUMP     the line search's inputs into the env slice, -DDUCK_AUX_LDS the whole slice
//                      into the aux record (tools/diag_lds.py)
#pragma once
#include "../../include/duck.h"

#define DUCK_NOTHING \
  do {               \
  } while (0)

// Stage and counter numbers: (number, identifier, "label"). STAGE_MARK(ST_x) adds the cycles since the
// previous mark (or since STAGE_T0 / STAGE_RESET) to counter x, STAGE_COUNT*(ST_N_x, v) adds v to an
// event counter. tools/stage_table.py reads this table from the text of this header: the tools take
// numbers, labels and DUCK_NSTAGE from here (how they group the stages is their own).
#define DUCK_NSTAGE 60
// clang-format off
#define DUCK_STAGE_TABLE(X) \
  X(0, KINEMATICS, "kinematics") \
  X(1, COM_POS, "com_pos") \
  X(2, RNE, "rne") \
  X(3, CRB, "crb") \
  X(4, SMOOTH_ACC, "qacc_smooth solve") \
  X(5, COLLISION, "collision") \
  X(6, MAKE_ROWS, "make_rows") \
  X(7, SOLVE, "solve") \
  X(8, SENSORS_EULER, "sensors+euler") \
  X(9, WARM_SELECT, "solve:warm costs+select") \
  X(10, NEWTON_DIR, "solve:newton_dir") \
  X(11, NEWTON_SPARSE, "solve:(dense fallback)") \
  X(12, SEARCH_PRODUCTS, "solve:jmul+mulM") \
  X(13, LINESEARCH, "solve:linesearch") \
  X(14, MODEL_COPY, "model-table copy") \
  X(15, ENV_HOT_STORE, "env: hot state store") \
  X(16, NEWTON_GRAD, "newton:grad+diag") \
  X(17, NEWTON_JDJ, "newton:+J'DJ") \
  X(18, NEWTON_FACTOR, "newton:+factor_solve") \
  X(19, CRB_SUMS, "crb:inertia sums") \
  X(20, LOAD_COLS, "M columns -> registers") \
  X(21, RNE_A, "rne:A vel/acc") \
  X(22, RNE_B, "rne:A+B forces") \
  X(23, N_DENSE_FALLBACK, "dense Newton fallbacks") \
  X(24, KIN_LOCAL, "kinematics:local") \
  X(25, WARM_PRODUCTS, "solve:warm J,M products") \
  X(26, COLLISION_FLOOR, "collision:floor") \
  X(27, N_FOOT_SAT, "foot/foot SAT runs") \
  X(28, SMOOTH, "smooth (actuation, damping)") \
  X(29, ENV_PRE, "env: pre-physics (per env-step)") \
  X(30, ENV_CONTACTS_OBS, "env: contacts+obs") \
  X(31, ENV_TERM, "env: termination+rewards+state") \
  X(32, ENV_HOT_LOAD, "env: hot state load") \
  X(33, ENV_RNG, "env: rng draws") \
  X(34, ENV_OBS_STORE, "env: obs/priv stores") \
  X(35, RNE_LIMB, "rne:C limb sums") \
  X(36, RNE_ROOT, "rne:C root sums") \
  X(37, HF_SCREEN, "hfield: setup+screen+silhouettes") \
  X(38, HF_QUEUE, "hfield: survivor queue") \
  X(39, HF_SLOTS, "hfield: slots") \
  X(40, N_HF_SURVIVORS, "hfield survivors") \
  X(41, HFQ_DESC, "queue: descriptors") \
  X(42, HFQ_SAT, "queue: per-lane SAT") \
  X(43, HFQ_GATHER, "queue: gather") \
  X(44, SAT_VERTICAL, "sat: vertical pairs") \
  X(45, SAT_PASS1, "sat: pass 1 (arc tests)") \
  X(46, N_HF_ROUNDS, "hfield queue rounds") \
  X(47, SAT_PASS2, "sat: pass 2 (crossing pairs)") \
  X(48, N_HF_PASS2_ITERS, "hfield pass-2 iterations") \
  X(49, N_HF_PAIRS, "hfield crossing pairs") \
  X(50, N_HF_EDGES, "hfield crossing edges") \
  X(51, N_HF_SURV_LE21, "hfield survivors per wave <=21") \
  X(52, N_HF_SURV_LE32, "hfield survivors per wave 22-32") \
  X(53, N_HF_SURV_LE42, "hfield survivors per wave 33-42") \
  X(54, N_HF_SURV_LE64, "hfield survivors per wave 43-64") \
  X(55, N_HF_SURV_GT64, "hfield survivors per wave >64") \
  X(56, N_LS_WAVE_ITERS, "line search iterations (wave)") \
  X(57, N_LS_TEAM_ITERS, "line search iterations (team)") \
  X(58, N_LS_SEARCHES, "line searches")
// clang-format on
enum StageId {
#define DUCK_STAGE_ENUM(n, id, label) ST_##id = n,
  DUCK_STAGE_TABLE(DUCK_STAGE_ENUM)
#undef DUCK_STAGE_ENUM
};
#define DUCK_STAGE_CHECK(n, id, label) static_assert(n >= 0 && n < DUCK_NSTAGE, "stage number " #id);
DUCK_STAGE_TABLE(DUCK_STAGE_CHECK)
#undef DUCK_STAGE_CHECK
// duck_debug_stage_cycles' buffer: the stage counters, then three per-wave blocks of 1024 words
static_assert(DUCK_STAGE_CYCLES_WORDS == DUCK_NSTAGE + 3 * 1024, "duck.h's stage-cycle buffer length");

// ---------------- stage cycle counters, event counters, kernel timing ----------------
#if defined(DUCK_STAGE_PROF) || defined(DUCK_WAVE_PROF) || defined(DUCK_LAT_PROF)
#define DUCK_ANY_PROF 1
// [0, DUCK_NSTAGE) stage counters; then per wave of the first 1024 (wave = 4 * workgroup +
// wave-in-workgroup) of the last step_kernel launch: clock64 cycles, wall-clock (s_memrealtime,
// 100 MHz) start, wall-clock end
static __device__ unsigned long long g_stage_cycles[DUCK_NSTAGE + 3 * 1024];
// the stage counters themselves are kept per workgroup slot (summed by the host): one shared
// counter per stage made every workgroup's atomics contend at one L2 channel, which slowed whole
// XCDs by up to 30 % in profiled runs
static __device__ unsigned long long g_stage_wg[DUCK_NSTAGE * 256];
#define STAGE_ADD(k, v) atomicAdd(&g_stage_wg[(k) * 256 + (blockIdx.x & 255)], (v))
// step_kernel's prologue and epilogue: each wave's cycles and wall-clock start and end
#define KERNEL_T0() const unsigned long long kstart_ = clock64(), kwall_ = wall_clock64()
#define KERNEL_T1()                                             \
  do {                                                          \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 256) {          \
      const int w_ = 4 * blockIdx.x + threadIdx.x / 64;         \
      g_stage_cycles[DUCK_NSTAGE + w_] = clock64() - kstart_;   \
      g_stage_cycles[DUCK_NSTAGE + 1024 + w_] = kwall_;         \
      g_stage_cycles[DUCK_NSTAGE + 2048 + w_] = wall_clock64(); \
    }                                                           \
  } while (0)
#else
#define KERNEL_T0() DUCK_NOTHING
#define KERNEL_T1() DUCK_NOTHING
#endif

// STAGE_T0() at the top of a function that marks stages; STAGE_MARK(ST_x) ends stage x
#if defined(DUCK_STAGE_PROF)
#define STAGE_T0() unsigned long long _t0 = wall_clock64(), _c0 = clock64()
#define STAGE_RESET() (_c0 = clock64())
#define STAGE_MARK(k)                                  \
  do {                                                 \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    const unsigned long long _c1 = clock64();          \
    if (threadIdx.x == 0) STAGE_ADD(k, _c1 - _c0);     \
    _c0 = _c1;                                         \
    (void)_t0;                                         \
  } while (0)
#elif defined(DUCK_LAT_PROF)
// latency-kernel builds: each stage's cycles summed over the launch in workgroup 0 (lane 0 of the
// wave that runs it; in the latency kernel every stage runs on one wave) into
// g_stage_cycles[DUCK_NSTAGE + 64 + k]; the waits between stages are outside every stage
#define STAGE_T0() unsigned long long _c0 = clock64()
#define STAGE_RESET() (_c0 = clock64())
#define STAGE_MARK(k)                                                                                         \
  do {                                                                                                        \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                        \
    const unsigned long long _c1 = clock64();                                                                 \
    if (blockIdx.x == 0 && ((int)threadIdx.x & 63) == 0) g_stage_cycles[DUCK_NSTAGE + 64 + (k)] += _c1 - _c0; \
    _c0 = _c1;                                                                                                \
  } while (0)
#else
#define STAGE_T0() DUCK_NOTHING
#define STAGE_RESET() DUCK_NOTHING
#ifdef DUCK_ASM_MARKS
// static instruction counts per stage: the comment "; STAGE_MARK ST_x" at each stage boundary, no code
#define STAGE_MARK(k) asm volatile("; STAGE_MARK " #k ::: "memory")
#else
#define STAGE_MARK(k) DUCK_NOTHING
#endif
#endif

#ifdef DUCK_ASM_MARKS
#define ASM_MARK(name) asm volatile("; " name ::: "memory")
#else
#define ASM_MARK(name) DUCK_NOTHING
#endif

// Event counters (-DDUCK_STAGE_PROF). STAGE_COUNT: every lane that gets here adds v to counter k;
// STAGE_COUNT_IF: the lanes for which c holds; STAGE_COUNT_WAVE0: one lane (the first active) of wave 0. STAGE_PROF_ONLY(code): code that only
// feeds a counter; `if constexpr (STAGE_PROF)` for a longer block of it.
#ifdef DUCK_STAGE_PROF
constexpr bool STAGE_PROF = true;
#define STAGE_PROF_ONLY(...) __VA_ARGS__
#define STAGE_COUNT_IF(c, k, v) \
  do {                          \
    if (c) STAGE_ADD(k, (v));   \
  } while (0)
#define STAGE_COUNT(k, v) STAGE_COUNT_IF(true, k, v)
#define STAGE_COUNT_WAVE0(k, v) \
  STAGE_COUNT_IF(threadIdx.x < 64 && (int)threadIdx.x == __ffsll((long long)__ballot(1)) - 1, k, v)
#else
constexpr bool STAGE_PROF = false;
#define STAGE_PROF_ONLY(...)
#define STAGE_COUNT_IF(c, k, v) DUCK_NOTHING
#define STAGE_COUNT(k, v) DUCK_NOTHING
#define STAGE_COUNT_WAVE0(k, v) DUCK_NOTHING
#endif

// behind duck_debug_stage_cycles: the counters into out[DUCK_STAGE_CYCLES_WORDS], the per-workgroup slots summed
static int stage_cycles_of(unsigned long long* out, int reset) {
#ifdef DUCK_ANY_PROF
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stage_cycles), sizeof(unsigned long long) * DUCK_STAGE_CYCLES_WORDS);
  static unsigned long long wg[DUCK_NSTAGE * 256];
  if (e == hipSuccess) e = hipMemcpyFromSymbol(wg, HIP_SYMBOL(g_stage_wg), sizeof(wg));
  for (int k = 0; k < DUCK_NSTAGE && e == hipSuccess; k++)
    for (int b = 0; b < 256; b++) out[k] += wg[k * 256 + b];
  if (e == hipSuccess && reset) {
    static unsigned long long z[DUCK_NSTAGE * 256 > DUCK_STAGE_CYCLES_WORDS ? DUCK_NSTAGE * 256 : DUCK_STAGE_CYCLES_WORDS] = {0};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_stage_cycles), z, sizeof(unsigned long long) * DUCK_STAGE_CYCLES_WORDS);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_stage_wg), z, sizeof(wg));
  }
  return e == hipSuccess ? 0 : DUCK_EHIP;
#else
  (void)out;
  (void)reset;
  return DUCK_EUNSUPPORTED;
#endif
}

// ---------------- latency-kernel event times ----------------
// -DDUCK_LAT_PROF: clock64 of cross-wave event slot k (tools/lat_prof.py names the slots) of substep 5 in
// workgroup 0, into the per-wave cycle slots of g_stage_cycles (which only the throughput kernel
// writes); LAT2_T: the paired kernel, its first pair of waves
#ifdef DUCK_LAT_PROF
#define LAT_T(k, s)                                                                                                 \
  do {                                                                                                              \
    if (blockIdx.x == 0 && ((int)threadIdx.x & 63) == 0 && (s) == 5) g_stage_cycles[DUCK_NSTAGE + (k)] = clock64(); \
  } while (0)
#define LAT2_T(k, s)                    \
  do {                                  \
    if (threadIdx.x < 128) LAT_T(k, s); \
  } while (0)
#else
#define LAT_T(k, s) DUCK_NOTHING
#define LAT2_T(k, s) DUCK_NOTHING
#endif

// ---------------- stage doubling ----------------
// -DDUCK_DOUBLE=k (tools/stage_pmc_summary.py, tools/gpu_stage_double.sh, tools/gpu_stage_pmc.sh,
// tools/gpu_sat_double.sh): one idempotent stage runs twice, and the launch-time (and counter)
// difference to the normal build is that stage's cost, unperturbed by markers. The values of k:
// clang-format off
#define DUCK_DOUBLE_TABLE(D) \
  D(1, "crb") \
  D(2, "collision") \
  D(3, "make_rows") \
  D(4, "smooth_acc (qacc_smooth factor + solves)") \
  D(5, "solve (warm start + Newton + line search)") \
  D(6, "kinematics") \
  D(7, "com_pos") \
  D(8, "rne + smooth") \
  D(9, "M's register columns") \
  D(11, "hf SAT pass 2") \
  D(12, "hf SAT pass 1") \
  D(13, "hf contact point") \
  D(14, "hf screen") \
  D(15, "hf vertical-edge pairs") \
  D(17, "hf silhouette lists") \
  D(18, "hf survivor descriptors") \
  D(19, "hf manifold slots + contact stores") \
  D(20, "hf hull-face axes") \
  D(21, "warm start") \
  D(22, "Newton direction (gradient, J'DJ, factor + solves)")
// clang-format on
//   STAGE_AGAIN(k, stmt);                         a call-shaped stage: stmt once more
//   STAGE_TWICE(k) { STAGE_FRESH(k, a, b); ... }  a block: two passes, with the float arrays a, b
//                                                 laundered so that the second pass is recomputed
//   STAGE_KEEP(k, x); STAGE_TWICE(k) { STAGE_RESTORE(k, x); ... }  a block that consumes the array x
#ifdef DUCK_DOUBLE
// values the compiler must treat as changed
template <int N>
__device__ __forceinline__ void launder(float (&x)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++) asm volatile("" : "+v"(x[i]));
}
template <int N, int M>
__device__ __forceinline__ void launder(float (&x)[N][M]) {
#pragma unroll
  for (int i = 0; i < N; i++) launder(x[i]);
}
template <class... A>
__device__ __forceinline__ void stage_fresh(A&... a) {
  (launder(a), ...);
}
template <class T, int N>
struct StageKept {
  T v[N];
};
template <class T, int N>
__device__ __forceinline__ StageKept<T, N> stage_keep(const T (&x)[N]) {
  StageKept<T, N> s;
  for (int i = 0; i < N; i++) s.v[i] = x[i];
  return s;
}
#define STAGE_AGAIN(k, ...)                            \
  do {                                                 \
    if constexpr (DUCK_DOUBLE == (k)) { __VA_ARGS__; } \
  } while (0)
// STAGE_TWICE(k) is the loop in the build that doubles k and nothing in every other (a loop of one pass
// would still shift the code of the other stages): chosen by name, STAGE_TWICE_k, for the blocks' k
#define STAGE_TWICE(k) STAGE_TWICE_##k
#define STAGE_TWO_PASSES for (int rep_ = 0; rep_ < 2; rep_++)
#if DUCK_DOUBLE == 11
#define STAGE_TWICE_11 STAGE_TWO_PASSES
#else
#define STAGE_TWICE_11
#endif
#if DUCK_DOUBLE == 12
#define STAGE_TWICE_12 STAGE_TWO_PASSES
#else
#define STAGE_TWICE_12
#endif
#if DUCK_DOUBLE == 13
#define STAGE_TWICE_13 STAGE_TWO_PASSES
#else
#define STAGE_TWICE_13
#endif
#if DUCK_DOUBLE == 14
#define STAGE_TWICE_14 STAGE_TWO_PASSES
#else
#define STAGE_TWICE_14
#endif
#if DUCK_DOUBLE == 15
#define STAGE_TWICE_15 STAGE_TWO_PASSES
#else
#define STAGE_TWICE_15
#endif
#if DUCK_DOUBLE == 17
#define STAGE_TWICE_17 STAGE_TWO_PASSES
#else
#define STAGE_TWICE_17
#endif
#if DUCK_DOUBLE == 18
#define STAGE_TWICE_18 STAGE_TWO_PASSES
#else
#define STAGE_TWICE_18
#endif
#if DUCK_DOUBLE == 19
#define STAGE_TWICE_19 STAGE_TWO_PASSES
#else
#define STAGE_TWICE_19
#endif
#if DUCK_DOUBLE == 20
#define STAGE_TWICE_20 STAGE_TWO_PASSES
#else
#define STAGE_TWICE_20
#endif
#define STAGE_FRESH(k, ...)                                      \
  do {                                                           \
    if constexpr (DUCK_DOUBLE == (k)) stage_fresh(__VA_ARGS__);  \
  } while (0)
#define STAGE_KEEP(k, x) const auto x##_kept_ = stage_keep(x)
#define STAGE_RESTORE(k, x)                                                                 \
  do {                                                                                      \
    if constexpr (DUCK_DOUBLE == (k))                                                       \
      for (int i_ = 0; i_ < (int)(sizeof(x) / sizeof(x[0])); i_++) x[i_] = x##_kept_.v[i_]; \
  } while (0)
#else
#define STAGE_AGAIN(k, ...) DUCK_NOTHING
#define STAGE_TWICE(k)
#define STAGE_FRESH(k, ...) DUCK_NOTHING
#define STAGE_KEEP(k, x) DUCK_NOTHING
#define STAGE_RESTORE(k, x) DUCK_NOTHING
#endif

// ---------------- line-search dumps, the aux record's slice tail ----------------
// per-lane dump slots after the Lay fields (TLay::SINK, 2 x TEAM words; the line-search dumps use 136)
#ifdef DUCK_LS_DUMP
constexpr int SINK_WORDS = 136;
// the line search's inputs, into the (dead) KC scratch of the env slice: at its start the wave's exec
// mask and the search direction; the lane's |search|^2 partial sum; the quadratic's coefficients
#define LS_DUMP_START(L, lane)                                          \
  do {                                                                  \
    const unsigned long long ex_ = __builtin_amdgcn_read_exec();        \
    L[TL::KC + 88 + lane] = __int_as_float((int)(ex_ & 0xffffffffull)); \
    L[TL::KC + 104 + lane] = __int_as_float((int)(ex_ >> 32));          \
    L[TL::KC + 120 + lane] = L[Ly::SRCH + lane];                        \
  } while (0)
#define LS_DUMP_NORM(L, lane, sn)        \
  do {                                   \
    L[TL::KC + 56 + lane] = (float)lane; \
    L[TL::KC + 72 + lane] = sn;          \
  } while (0)
#define LS_DUMP_QUAD(L, lane, q0, q1, q2, G0, G1, G2, gtol, sn)                                                          \
  do {                                                                                                                   \
    L[TL::KC + 8 + 3 * lane] = q0; L[TL::KC + 9 + 3 * lane] = q1; L[TL::KC + 10 + 3 * lane] = q2;                        \
    if (lane == 0) { L[TL::KC] = G0; L[TL::KC + 1] = G1; L[TL::KC + 2] = G2; L[TL::KC + 3] = gtol; L[TL::KC + 4] = sn; } \
  } while (0)
#else
constexpr int SINK_WORDS = 32;
#define LS_DUMP_START(L, lane) DUCK_NOTHING
#define LS_DUMP_NORM(L, lane, sn) DUCK_NOTHING
#define LS_DUMP_QUAD(L, lane, q0, q1, q2, G0, G1, G2, gtol, sn) DUCK_NOTHING
#endif
// -DDUCK_AUX_LDS: the aux record (Phys::write_aux) ends with the whole env slice, Lay fields + dump slots
#ifdef DUCK_AUX_LDS
constexpr bool AUX_LDS = true;
#else
constexpr bool AUX_LDS = false;
#endif
