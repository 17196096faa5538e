// duck_physics.h — per-env LDS layout and shared physics helpers of the MI355X Open Duck kernels.
//
// The fused mjx.step itself (kinematics -> com/cinert/cdof -> RNE -> CRB -> actuation/passive ->
// smooth acceleration -> collision -> constraint rows -> MJX Newton -> sensors -> Euler) is the
// 16-lane team implementation in duck_team.h. This header holds what it builds on: the per-env LDS
// slice layout (Lay), the impedance law (kbi), the plane/convex manifold helpers, and a few per-env
// helpers (Phys).
//
// Contact Jacobians are never materialised: a contact row is a 6-vector a = [r x u; u]
// in the foot's com-based spatial frame, J.x = a . (sum_chain cdof_i x_i), and J'DJ is
// accumulated as one 6x6 block per foot projected onto the foot's dof chain.
#pragma once
#include "../../include/duck_env.h"
#include "duck_math.h"
#include "duck_measure.h"

#define DNI __device__ __noinline__
// compiler-only barrier: stops the scheduler from hoisting a whole unrolled loop's LDS
// loads into registers at once (which spills); costs no instruction
#define SCHED_FENCE() asm volatile("" ::: "memory")

// LDS-qualified pointer: keeps every slice access a ds_read/ds_write (a generic float*
// passed into a non-inlined stage would compile to flat_load/flat_store through the
// vector-memory pipe)
typedef __attribute__((address_space(3))) float lds_float;
// The alignment contract of the dynamic LDS: every declaration of it is 16-byte aligned, every env
// slice starts a multiple of 4 floats into it (TLay: STRIDE % 4 == 0), and env_slice() says so, so a
// run of 2 / 4 words that starts at an even / 4-aligned Lay offset is one ds_read_b64 / _b128 with a
// 16-bit byte offset instead of ds_read2_b32s behind a v_add_u32 (their offsets reach 1020 B only).
// A wide access off its alignment does not fault, it replays (SQ_LDS_UNALIGNED_STALL): a pointer
// that is not a slice base + a compile-time offset must not carry the assumption (the staged hot
// state, ESTRIDE odd).
#define LDS_ALIGNED __attribute__((aligned(16)))
DK lds_float* lds_assume16(lds_float* p) {
  __builtin_assume(((unsigned)(__SIZE_TYPE__)p & 15u) == 0u);
  return p;
}

// the longest privileged observation row (Joystick with imitation: duck_layout_make's priv_size);
// the state row is its prefix (write_obs_team, duck_env_kernels.h)
constexpr int priv_row_max(int nu) { return DUCK_OBS_SIZE(nu) + 15 + 3 * nu + 1 + 2 + 6 + 2 + 40 + 1 + 2; }

// What a workgroup's 160 KB of LDS holds next to the throughput kernel's 16 env slices decides how much
// padding a slice may carry: lay_keeps() says, for slices of `total` words, whether the model blob
// (bit 0), else the hull SAT tables (bit 1), and the staged hot state (bit 2) stay in LDS, or -1 when
// the slices alone do not fit. The same sums as TLay<Md, 0> (duck_team.h), which asserts that they agree.
constexpr int LDS_WORDS = 160 * 1024 / 4;
constexpr int SLICES_WG = 16;  // env slices per throughput workgroup (= TEAM_WG)
// (SINK_WORDS: the per-lane dump slots after the Lay fields, TLay::SINK; duck_measure.h)
constexpr int slice_stride(int used) { return ((used + 15) / 32) * 32 + 16; }  // = 16 (mod 32), >= used
// step_kernel's staged hot state (the duck_layout fields before first_qpos) + the step's 64 random draws
template <class Md>
constexpr int hot_words() { return Md::NQ + 2 * Md::NV + 8 * Md::NU + 77; }
constexpr int hot_stride(int hot) { return (hot + 64) | 1; }  // odd: distinct banks
template <class Md>
constexpr int lay_keeps(int total) {
  const int tab = SLICES_WG * slice_stride(total + SINK_WORDS);
  const int nht = Md::B_HEND > Md::B_HFACE ? Md::B_HEND - Md::B_HFACE : 0;
  const bool tabl = tab + Md::NBLOB <= LDS_WORDS, htl = !tabl && nht > 0 && tab + nht <= LDS_WORDS;
  const int es = tab + (tabl ? Md::NBLOB : (htl ? nht : 0));
  const bool esl = es + SLICES_WG * hot_stride(hot_words<Md>()) <= LDS_WORDS;
  return es > LDS_WORDS ? -1 : tabl + 2 * htl + 4 * esl;
}

// Per-env LDS slice layout (floats); a slice is contiguous and addressed through an lds_float*.
//
// Order and padding serve the alignment contract (LDS_ALIGNED above): the fields whose records a lane
// reads or writes whole -- poses, frames, inertias, 6-vectors, the tree passes' scratch, the constraint
// rows' records -- come first and start on 4-float boundaries, the lane-indexed vectors (state,
// per-env model values), which gain nothing from alignment, come last. Most boundaries fall out of
// the sizes (4 NB, 10 NB, 6 NB, 6 NV, 18 + NM + 1 with NM odd ...); where one does not, a4() / a2()
// pad up to AL floats. A scene gets the even record strides (WIDE) and AL = 4 where such slices leave
// in LDS what packed ones do (lay_keeps), else what of it fits (lay_rule): rough + backlash has 9 words
// a slice to spare, and the same order without padding still puts most records on their boundaries.
template <class Md, int AL, bool WIDE>
struct LayT {
  static constexpr int ALIGN = AL, WIDE_RECORDS = WIDE;
  static constexpr int NB = Md::NB, NV = Md::NV, NQ = Md::NQ, NU = Md::NU;
  static constexpr int NCON = 4 * Md::NPAIR;
  static constexpr int R_LIM = Md::NFRIC, R_CON = Md::NFRIC + Md::NLIM;
  static constexpr int NROW = R_CON + 4 * NCON;
  static constexpr int up(int x, int a) { return (x + a - 1) / a * a; }
  static constexpr int a4(int x) { return up(x, AL < 4 ? AL : 4); }  // 16-byte fields
  static constexpr int a2(int x) { return up(x, AL < 2 ? AL : 2); }  // 8-byte fields
  // a per-row array whose contact rows (4 per contact, from R_CON on) start on a 4-float boundary
  static constexpr int arow(int x) { return a4(x + R_CON) - R_CON; }
  // record strides of the fields indexed per lane (words per body / per contact slot): body positions,
  // body frames, contact points, contact frames. WIDE: even, so that a lane's record is ds_read_b64 /
  // _b128s (3 -> 4 and 9 -> 10 words: 60 more words a slice); else packed and odd (conflict-free banks
  // over the lanes of a team, b32 accesses only). DESIGN.md §3 has the counts and the measurements.
  static constexpr int XPS = WIDE ? 4 : 3, XMS = WIDE ? 10 : 9, CRS = WIDE ? 4 : 3, CFS = WIDE ? 10 : 9;
  // bodies
  static constexpr int XQ = 0, XMAT = XQ + 4 * NB, XPOS = a4(XMAT + XMS * NB), CIN = a4(XPOS + XPS * NB);
  static constexpr int CVEL = a4(CIN + 10 * NB), CDOF = a4(CVEL + 6 * NB);
  // matrices
  // M, then one word kept at zero (crb writes it with M): the register column
  // loads of M read it for the entries outside the tree pattern (codegen mcolz table)
  static constexpr int M = a4(CDOF + 6 * NV), MZERO = M + Md::NM, CDD1 = a2(MZERO + 1);
  // the subtree centre of mass, then the small outputs of the last forward (3 + 3 + 2 + 2 + 2 words)
  static constexpr int COM = a4(CDD1 + 18), IMUR = COM + 3, OCON = IMUR + 3, FOOTZ = OCON + 2, FLAGS = FOOTZ + 2;
  static constexpr int H = a4(FLAGS + 2);
  // H: scratch in front of the constraint rows, dead outside the stage that uses it together with
  // the rows (the Newton Hessian itself is assembled in registers, never stored). Its users, each
  // from H on: the tree passes' scratch (rne: 12 NB + 6 NV), the hull/hull SAT's edge tables (6 per
  // hull edge and face), the height-field survivor queue (16 entries of 28 per env slice + 16-B
  // alignment), the staged privileged observation row (env code, priv_row_max). H is sized so that
  // H + rows covers the largest of them: the rows alone cover most, so H is short (the backlash
  // scenes' slices then leave LDS for the model blob: TLay::TAB_LDS).
  static constexpr int SCR_TREE = 12 * NB + 6 * NV, SCR_SAT = 6 * (Md::NHE + Md::NHF);
  static constexpr int SCR_HF = Md::FLOOR_TYPE == 1 ? 3 + 28 * 16 : 0, SCR_OBS = priv_row_max(NU);
  static constexpr int cmax(int a, int b) { return a > b ? a : b; }
  static constexpr int SCR_NEED = cmax(cmax(SCR_TREE, SCR_SAT), cmax(SCR_HF, SCR_OBS));
  static constexpr int HSZ = ((cmax(SCR_NEED - 4 * NROW - Md::NLIM, 0) + 3) / 4) * 4;
  static constexpr int JA = arow(H + HSZ), JV = arow(JA + NROW), RD = arow(JV + NROW), AREF = arow(RD + NROW);
  static constexpr int LSGN = a2(AREF + NROW);
  static constexpr int CR = a4(LSGN + Md::NLIM), CFR = a4(CR + CRS * NCON), CDIST = a4(CFR + CFS * NCON);
  static_assert(CR - H >= SCR_NEED, "H + rows must cover the scratch users");
  // Newton 6x6 foot blocks live in CIN's storage (composite inertias are dead after crb())
  static constexpr int KL = CIN, KR = a2(KL + 21), KLR = a2(KR + 21), FL = KLR + 36, FR = FL + 6;
  static_assert(FR + 6 <= CIN + 10 * NB, "Newton blocks must fit in CIN");
  // larger outputs of the last forward
  static constexpr int AF = a2(CDIST + NCON), SENS = a2(AF + NU);
  // state
  static constexpr int QPOS = SENS + Md::NSENSORDATA, QVEL = QPOS + NQ, WARM = QVEL + NV, CTRL = WARM + NV;
  static constexpr int QACC = CTRL + NU;
  static constexpr int QSM = QACC + NV, FSM = QSM + NV, SRCH = FSM + NV, GRAD = SRCH + NV, MA = GRAD + NV;
  // per-env model values (domain randomisation), contiguous in the order of the model blob's nominal block
  static constexpr int DMASS = MA + NV, DIPOS = DMASS + NB, DARM = DIPOS + 3, DFRIC = DARM + NV;
  static constexpr int DQ0 = DFRIC + NV, DKP = DQ0 + NQ;
  static constexpr int TOTAL = a4(DKP + NU);
  // what the layout promises the compiler's alignment analysis (each holds for AL = 4)
  static_assert(AL < 4 || (XQ % 4 == 0 && XMAT % 4 == 0 && CIN % 4 == 0 && CVEL % 4 == 0 && CDOF % 4 == 0 && M % 4 == 0 &&
                           COM % 4 == 0 && H % 4 == 0 && (JA + R_CON) % 4 == 0 && (JV + R_CON) % 4 == 0 &&
                           (RD + R_CON) % 4 == 0 && (AREF + R_CON) % 4 == 0 && CR % 4 == 0 && CFR % 4 == 0 &&
                           CDIST % 4 == 0 && TOTAL % 4 == 0),
                "16-byte fields");
  static_assert(AL < 2 || (XPOS % 2 == 0 && CDD1 % 2 == 0 && KR % 2 == 0 && KLR % 2 == 0 && FL % 2 == 0 && FR % 2 == 0 &&
                           LSGN % 2 == 0 && AF % 2 == 0 && SENS % 2 == 0),
                "8-byte fields");
};
// the layout rule a scene affords: the first of (WIDE, AL) = (1, 4), (1, 2), (1, 1), (0, 4), (0, 2), (0, 1)
// whose slices keep in LDS what the packed slices (0, 1) keep; returned as 8 WIDE + AL
template <class Md>
constexpr int lay_rule() {
  constexpr int keep = lay_keeps<Md>(LayT<Md, 1, false>::TOTAL);
  if (lay_keeps<Md>(LayT<Md, 4, true>::TOTAL) == keep) return 8 + 4;
  if (lay_keeps<Md>(LayT<Md, 2, true>::TOTAL) == keep) return 8 + 2;
  if (lay_keeps<Md>(LayT<Md, 1, true>::TOTAL) == keep) return 8 + 1;
  return lay_keeps<Md>(LayT<Md, 4, false>::TOTAL) == keep ? 4 : (lay_keeps<Md>(LayT<Md, 2, false>::TOTAL) == keep ? 2 : 1);
}
template <class Md>
struct Lay : LayT<Md, lay_rule<Md>() & 7, (lay_rule<Md>() >> 3) != 0> {};

// solref/solimp -> (k, b, imp) (mjx constraint._kbi / MuJoCo mj_makeImpedance)
DK void kbi(const float* solref, const float* solimp, float pos, float dt, float& k, float& b, float& imp) {
  const float timeconst = fmaxf(solref[0], 2.0f * dt);
  const float dampratio = solref[1];
  const float dmin = fminf(fmaxf(solimp[0], 0.0001f), 0.9999f), dmax = fminf(fmaxf(solimp[1], 0.0001f), 0.9999f);
  const float width = fmaxf(1e-15f, solimp[2]), mid = fminf(fmaxf(solimp[3], 0.0001f), 0.9999f);
  const float power = fmaxf(1.0f, solimp[4]);
  k = 1.0f / (dmax * dmax * timeconst * timeconst * dampratio * dampratio);
  b = 2.0f / (dmax * timeconst);
  const float x = fabsf(pos) / width;
  float y;
  if (power == 2.0f) {
    const float ya = (1.0f / mid) * x * x;
    const float yb = 1.0f - (1.0f / (1.0f - mid)) * (1.0f - x) * (1.0f - x);
    y = x < mid ? ya : yb;
  } else {
    const float ya = (1.0f / powf(mid, power - 1.0f)) * powf(x, power);
    const float yb = 1.0f - (1.0f / powf(1.0f - mid, power - 1.0f)) * powf(1.0f - x, power);
    y = x < mid ? ya : yb;
  }
  float im = dmin + y * (dmax - dmin);
  im = fminf(fmaxf(im, dmin), dmax);
  imp = x > 1.0f ? dmax : im;
}

// argmax with a tie band (first index within tol of the max) — same rule as the oracle
template <int N>
DK int argmax_tol(const float* v, float tol) {
  float mx = v[0];
#pragma unroll
  for (int i = 1; i < N; i++) mx = fmaxf(mx, v[i]);
  int r = N - 1;
#pragma unroll
  for (int i = N - 1; i >= 0; i--) r = (v[i] >= mx - tol) ? i : r;
  return r;
}
#define MANIFOLD_TOL 2e-8f

template <int N>
DK void pick3(const float (*P)[3], int k, float* out) {
  out[0] = P[0][0]; out[1] = P[0][1]; out[2] = P[0][2];
#pragma unroll
  for (int i = 1; i < N; i++) {
    const bool s = (i == k);
    out[0] = s ? P[i][0] : out[0];
    out[1] = s ? P[i][1] : out[1];
    out[2] = s ? P[i][2] : out[2];
  }
}
template <int N>
DK float pick1(const float* P, int k) {
  float o = P[0];
#pragma unroll
  for (int i = 1; i < N; i++) o = (i == k) ? P[i] : o;
  return o;
}

// mjx collision_convex._manifold_points: 4 polygon points of ~maximal area
template <int N>
DK void manifold_points(const float (*poly)[3], const bool* mask, const float* nrm, int idx[4]) {
  float dm[N], s[N], s2[2 * N];
#pragma unroll
  for (int k = 0; k < N; k++) dm[k] = mask[k] ? 0.0f : -1e6f;
  const int a = argmax_tol<N>(dm, 0.0f);
  float pa[3];
  pick3<N>(poly, a, pa);
#pragma unroll
  for (int k = 0; k < N; k++) {
    const float dx = pa[0] - poly[k][0], dy = pa[1] - poly[k][1], dz = pa[2] - poly[k][2];
    s[k] = dx * dx + dy * dy + dz * dz + dm[k];
  }
  const int b = argmax_tol<N>(s, MANIFOLD_TOL);
  float pb[3];
  pick3<N>(poly, b, pb);
  float amb[3] = {pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]}, ab[3];
  cross3(ab, nrm, amb);
#pragma unroll
  for (int k = 0; k < N; k++) {
    const float ap[3] = {pa[0] - poly[k][0], pa[1] - poly[k][1], pa[2] - poly[k][2]};
    s[k] = fabsf(dot3(ap, ab)) + dm[k];
  }
  const int c = argmax_tol<N>(s, MANIFOLD_TOL);
  float pc[3];
  pick3<N>(poly, c, pc);
  float amc[3] = {pa[0] - pc[0], pa[1] - pc[1], pa[2] - pc[2]};
  float bmc[3] = {pb[0] - pc[0], pb[1] - pc[1], pb[2] - pc[2]};
  float ac[3], bc[3];
  cross3(ac, nrm, amc);
  cross3(bc, nrm, bmc);
#pragma unroll
  for (int k = 0; k < N; k++) {
    const float bp[3] = {pb[0] - poly[k][0], pb[1] - poly[k][1], pb[2] - poly[k][2]};
    const float ap[3] = {pa[0] - poly[k][0], pa[1] - poly[k][1], pa[2] - poly[k][2]};
    s2[k] = fabsf(dot3(bp, bc)) + dm[k];
    s2[N + k] = fabsf(dot3(ap, ac)) + dm[k];
  }
  int d = argmax_tol<2 * N>(s2, MANIFOLD_TOL);
  d = d >= N ? d - N : d;
  idx[0] = a; idx[1] = b; idx[2] = c; idx[3] = d;
}

// mjx math.make_frame: rows (n, t1, t2)
DK void make_frame(float* fr, const float* nin) {
  float n[3] = {nin[0], nin[1], nin[2]};
  const float nn = sqrtf(dot3(n, n));
  if (nn > 1e-15f) { n[0] /= nn; n[1] /= nn; n[2] /= nn; }
  float b[3];
  const bool y = (-0.5f < n[1]) && (n[1] < 0.5f);
  b[0] = 0.0f; b[1] = y ? 1.0f : 0.0f; b[2] = y ? 0.0f : 1.0f;
  const float nb = dot3(n, b);
  b[0] -= n[0] * nb; b[1] -= n[1] * nb; b[2] -= n[2] * nb;
  const float bn = sqrtf(dot3(b, b));
  if (bn > 1e-15f) { b[0] /= bn; b[1] /= bn; b[2] /= bn; }
  float c[3];
  cross3(c, n, b);
  fr[0] = n[0]; fr[1] = n[1]; fr[2] = n[2];
  fr[3] = b[0]; fr[4] = b[1]; fr[5] = b[2];
  fr[6] = c[0]; fr[7] = c[1]; fr[8] = c[2];
}

template <class Md>
DK constexpr int cgeom_slot(int g) {
  return g == Md::FLOOR_GEOM ? 0 : (g == Md::LFOOT_GEOM ? 1 : 2);
}

// Per-env helpers of the team kernels (duck_team.h) and the env kernels: nominal per-env model
// values, collision geom frames, contact records, contact point velocity, the debug aux record.
template <class Md>
struct Phys {
  using Ly = Lay<Md>;
  static constexpr int NV = Md::NV, NB = Md::NB, NQ = Md::NQ, NU = Md::NU;
  static constexpr int NCON = Ly::NCON;

  // ---------------- per-env model values ----------------
  static DK void set_nominal(lds_float* L) {
#pragma unroll
    for (int b = 0; b < NB; b++) L[Ly::DMASS + b] = Md::body_mass[b];
#pragma unroll
    for (int k = 0; k < 3; k++) L[Ly::DIPOS + k] = Md::body_ipos[1][k];
#pragma unroll
    for (int i = 0; i < NV; i++) { L[Ly::DARM + i] = Md::dof_armature[i]; L[Ly::DFRIC + i] = Md::dof_frictionloss[i]; }
#pragma unroll
    for (int i = 0; i < NQ; i++) L[Ly::DQ0 + i] = Md::qpos0[i];
#pragma unroll
    for (int a = 0; a < NU; a++) L[Ly::DKP + a] = Md::actuator_kp[a];
  }

  // ---------------- collision (mjx collision_driver, 4 slots per pair) ----------------
  static DK void geom_frame(lds_float* L, int g, float* gp, float* gR) {
    const int b = Md::cgeom_body[g];
    if (Md::body_weldid[b] == 0) {
      float bq[4] = {Md::body_quat[b][0], Md::body_quat[b][1], Md::body_quat[b][2], Md::body_quat[b][3]}, BR[9], t[3];
      q2m(BR, bq);
      mulmv3(t, BR, Md::geom_pos[g]);
#pragma unroll
      for (int k = 0; k < 3; k++) gp[k] = Md::body_pos[b][k] + t[k];
      mulmm3(gR, BR, Md::geom_mat[g]);
    } else {
      float R[9], t[3];
#pragma unroll
      for (int k = 0; k < 9; k++) R[k] = L[Ly::XMAT + Ly::XMS * b + k];
      mulmv3(t, R, Md::geom_pos[g]);
#pragma unroll
      for (int k = 0; k < 3; k++) gp[k] = L[Ly::XPOS + Ly::XPS * b + k] + t[k];
      mulmm3(gR, R, Md::geom_mat[g]);
    }
  }

  static DK void store_contact(lds_float* L, int slot, float dist, const float* pos, const float* fr) {
    L[Ly::CDIST + slot] = dist;
#pragma unroll
    for (int a = 0; a < 3; a++) L[Ly::CR + Ly::CRS * slot + a] = pos[a] - L[Ly::COM + a];
#pragma unroll
    for (int a = 0; a < 9; a++) L[Ly::CFR + Ly::CFS * slot + a] = fr[a];
  }

  // ---------------- constraint rows (mjx make_constraint) ----------------
  static DK void contact_vel(const float* Sp, const float* r, float* v) {
    float t[3];
    cross3(t, Sp, r);
    v[0] = Sp[3] + t[0]; v[1] = Sp[4] + t[1]; v[2] = Sp[5] + t[2];
  }

  // debug record: qacc, qacc_smooth, qvel (pre-integration), qfrc_smooth, actuator_force,
  // sensordata, con_dist, con_pos, con_normal, M
  static DNI void write_aux(lds_float* L, float* aux, int stride) {
    int o = 0;
    for (int i = 0; i < NV; i++) aux[(o++) * stride] = L[Ly::QACC + i];
    for (int i = 0; i < NV; i++) aux[(o++) * stride] = L[Ly::QSM + i];
    for (int i = 0; i < NV; i++) aux[(o++) * stride] = L[Ly::QVEL + i];
    for (int i = 0; i < NV; i++) aux[(o++) * stride] = L[Ly::FSM + i];
    for (int a = 0; a < NU; a++) aux[(o++) * stride] = L[Ly::AF + a];
    for (int k = 0; k < Md::NSENSORDATA; k++) aux[(o++) * stride] = L[Ly::SENS + k];
    for (int s = 0; s < NCON; s++) aux[(o++) * stride] = L[Ly::CDIST + s];
    for (int s = 0; s < NCON; s++)
      for (int a = 0; a < 3; a++) aux[(o++) * stride] = L[Ly::CR + Ly::CRS * s + a] + L[Ly::COM + a];
    for (int s = 0; s < NCON; s++)
      for (int a = 0; a < 3; a++) aux[(o++) * stride] = L[Ly::CFR + Ly::CFS * s + a];  // contact normal
    for (int k = 0; k < Md::NM; k++) aux[(o++) * stride] = L[Ly::M + k];
    // debug builds: the whole env slice (Lay fields + the per-lane dump slots; tools/diag_lds.py)
    if constexpr (AUX_LDS)
      for (int k = 0; k < Ly::TOTAL + SINK_WORDS; k++) aux[(o++) * stride] = L[k];
  }
};

template <class Md>
constexpr int aux_size() {
  return 4 * Md::NV + Md::NU + Md::NSENSORDATA + 7 * Lay<Md>::NCON + Md::NM + (AUX_LDS ? Lay<Md>::TOTAL + SINK_WORDS : 0);
}
