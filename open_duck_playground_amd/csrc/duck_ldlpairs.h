// duck_ldlpairs.h — which row updates of the register LDL' go two to a packed FMA (compile time, from the
// dof tree).
//
// Pivot K of the factorization (TPhys::fac_pass) updates each lane's column at every ancestor row I of K,
//   H[I][c] -= t_I H[K][c],   t_I = H[K][I] / H[K][K],
// for the column sets s that reach row I (16 s <= I). Two such updates at the adjacent rows 2m and 2m + 1
// are one v_pk_fma_f32 over the register pair (col[2m], col[2m+1]) with the pair (t_2m, t_2m+1) and a
// splat of H[K][c]: each half is the fused multiply-add the scalar update is, so no bit moves. A pair
// needs both rows to be ancestors of K and both inside the set's range; 16 s is even, so 16 s <= 2m
// covers 2m + 1 as well. Every other update stays a scalar FMA. Plain C++ over Md::dof_parentid: a host
// program that includes a generated model header prints the table (tests/test_ldl_pairs_host.py).
#pragma once

// The scenes whose factorization takes the packed form. -DDUCK_LDL_PAIRS_OFF (a measurement build): none.
template <class Md>
constexpr bool ldl_pairs() {
#ifdef DUCK_LDL_PAIRS_OFF
  return false;
#else
  return true;
#endif
}

template <class Md, int TEAMW = 16>
struct LdlPairs {
  static constexpr int NV = Md::NV, NC = (NV + TEAMW - 1) / TEAMW;
  static constexpr bool ON = ldl_pairs<Md>();
  // a is a strict ancestor of dof d
  static constexpr bool anc(int a, int d) {
    for (int j = Md::dof_parentid[d]; j >= 0; j = Md::dof_parentid[j])
      if (j == a) return true;
    return false;
  }
  // pivot k updates row i of column set s at all
  static constexpr bool upd(int k, int i, int s) { return i >= 0 && i < NV && anc(i, k) && TEAMW * s <= i; }
  // ... as the low half (row i = 2m) of a packed update of rows 2m, 2m + 1
  static constexpr bool lo(int k, int i, int s) { return ON && i % 2 == 0 && upd(k, i, s) && upd(k, i + 1, s); }
  // ... as its high half (row i = 2m + 1): done with row i - 1, no code of its own
  static constexpr bool hi(int k, int i, int s) { return i % 2 == 1 && lo(k, i - 1, s); }
};
