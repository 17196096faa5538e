// Prints the compile-time pairing table of the register LDL' row updates (csrc/duck_ldlpairs.h) for one model
// header, with the header's own dof tree (tests/test_ldl_pairs_host.py). For every pivot k and column set s:
// the rows the pivot updates as the low half of a packed FMA, as its high half, and alone.
// Host C++ only: cc -std=c++17 -D__device__= -D__forceinline__=inline -DMODEL_HEADER='"..."' -DMODEL=DuckModel_x
#include <cstdio>
#ifdef MODEL_HEADER
#include MODEL_HEADER
#else
// an edited tree no shipped scene has: a free joint, a 3-dof limb, a 1-dof limb on the limb's first dof, and
// a 9-dof limb that crosses the boundary between the column sets at an odd row
struct EditedTree {
  static constexpr int NV = 19;
  static constexpr int dof_parentid[NV] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 10, 11, 12, 13, 14, 15, 16, 17};
};
#define MODEL EditedTree
#endif
#include "duck_ldlpairs.h"

int main() {
  using Md = MODEL;
  using LP = LdlPairs<Md, 16>;
  std::printf("NV %d NC %d on %d\nparent", Md::NV, LP::NC, (int)LP::ON);
  for (int i = 0; i < Md::NV; i++) std::printf(" %d", Md::dof_parentid[i]);
  std::printf("\n");
  for (int k = 0; k < Md::NV; k++)
    for (int s = 0; s < LP::NC; s++) {
      std::printf("pivot %d set %d lo", k, s);
      for (int i = 0; i < Md::NV; i++)
        if (LP::lo(k, i, s)) std::printf(" %d", i);
      std::printf(" hi");
      for (int i = 0; i < Md::NV; i++)
        if (LP::hi(k, i, s)) std::printf(" %d", i);
      std::printf(" single");
      for (int i = 0; i < Md::NV; i++)
        if (LP::upd(k, i, s) && !LP::lo(k, i, s) && !LP::hi(k, i, s)) std::printf(" %d", i);
      std::printf("\n");
    }
  return 0;
}
