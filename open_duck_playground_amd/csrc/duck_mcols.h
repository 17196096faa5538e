// duck_mcols.h — the pattern of M's register columns (compile time, from the dof tree).
//
// The solver holds the symmetric tree-sparse M as full columns in registers: lane l of column set s
// holds column c = 16 s + l (TPhys::load_cols). Its entry of row r is one of
//   the descendant form   M[r][c] = cdof_c . F_r   r = c or r a descendant of c   (F_r broadcast from lane r)
//   the ancestor form     M[c][r] = cdof_r . F_c   r an ancestor of c             (cdof_r broadcast from lane r)
//   zero                  otherwise (and for columns past NV)
// with F_i = Ic_body(i) cdof_i (crb() computes each entry once, in the row of the descendant, and the
// columns get both triangles through LDS). The kernel uses zero_row(): a row that is zero on every
// lane of a set is skipped by M x. The two forms' lane masks are what a build of the columns in
// registers needs (measured and not kept; tools/patches/mcols_register_build.patch applies to this tree
// and uses dmask, amask, thresh and depth). Plain C++ over
// Md::dof_parentid: a host program that includes a generated model header prints the table
// (tests/test_mcols_pattern_host.py).
#pragma once

// The scenes whose throughput kernel takes the two lean steps (crb's lane masks formed inside the substep,
// M x without the all-zero rows). The condition is a proxy in NV, not a measured property of a tree: a last
// column set of at most 4 columns, the shape crb() handles by its SPLIT form (the Open Duck scenes without
// backlash, NV = 20). What was measured, three alternating runs against the parent on one box: the shipped
// NV = 20 scenes C2 +1.5 %, C3 +1.5 %, C4 +0.4 % (inside its spread); rough + backlash (NV = 30, two sets
// in crb()'s full form) with both steps C5 -1.2 % (10.11-10.16 against 10.25-10.29 M env-steps/s), so the
// NV = 30 scenes keep the parent's code (profiles/r11_mcols_ab.txt, which also has the flat + backlash
// line). An edited model with NV of 17-20 takes the steps unmeasured: they move no bit, only time.
// -DDUCK_MCOLS_LEAN_ALL (a measurement build): every scene takes them.
template <class Md>
constexpr bool mcols_lean() {
#ifdef DUCK_MCOLS_LEAN_ALL
  return true;
#else
  return Md::NV > 16 && Md::NV % 16 != 0 && Md::NV % 16 <= 4;
#endif
}

template <class Md, int TEAMW = 16>
struct MCols {
  static constexpr int NV = Md::NV, NC = (NV + TEAMW - 1) / TEAMW;
  // a is a strict ancestor of dof d
  static constexpr bool anc(int a, int d) {
    for (int j = Md::dof_parentid[d]; j >= 0; j = Md::dof_parentid[j])
      if (j == a) return true;
    return false;
  }
  // number of strict ancestors of dof r (= the diagonal's position in the row's ancestor chain)
  static constexpr int depth(int r) {
    int n = 0;
    for (int j = Md::dof_parentid[r]; j >= 0; j = Md::dof_parentid[j]) n++;
    return n;
  }
  // lanes of set s whose entry of row r takes the descendant form (bit l: column 16 s + l)
  static constexpr unsigned dmask(int r, int s) {
    unsigned m = 0;
    for (int l = 0; l < TEAMW; l++) {
      const int c = TEAMW * s + l;
      if (c < NV && (c == r || anc(c, r))) m |= 1u << l;
    }
    return m;
  }
  // ... the ancestor form
  static constexpr unsigned amask(int r, int s) {
    unsigned m = 0;
    for (int l = 0; l < TEAMW; l++) {
      const int c = TEAMW * s + l;
      if (c < NV && anc(r, c)) m |= 1u << l;
    }
    return m;
  }
  // lanes of set s that hold a column of M
  static constexpr unsigned vmask(int s) {
    unsigned m = 0;
    for (int l = 0; l < TEAMW; l++)
      if (TEAMW * s + l < NV) m |= 1u << l;
    return m;
  }
  // valid lanes whose entry of row r is zero (neither form)
  static constexpr unsigned zmask(int r, int s) { return vmask(s) & ~(dmask(r, s) | amask(r, s)); }
  // row r of set s is zero on every lane: no code, and M x skips it
  static constexpr bool zero_row(int r, int s) { return (dmask(r, s) | amask(r, s)) == 0u; }
  // the lane at and below which a row's lanes take the descendant form (columns c <= r), above it the
  // ancestor form: 15 for a set left of the row's own, -1 for a set right of it
  static constexpr int thresh(int r, int s) { return s < r / TEAMW ? TEAMW - 1 : (s > r / TEAMW ? -1 : r % TEAMW); }
};
