// Prints the compile-time pattern table of M's register columns (csrc/duck_mcols.h) for one model
// header, with the header's own dof tree and M address table (tests/test_mcols_pattern_host.py).
// Host C++ only: cc -std=c++17 -D__device__= -D__forceinline__=inline -DMODEL_HEADER='"..."' -DMODEL=DuckModel_x
#include <cstdio>
#ifdef MODEL_HEADER
#include MODEL_HEADER
#else
// an edited tree no shipped scene has: a free joint, a 3-dof limb, a 1-dof limb on the limb's first dof, and
// a 9-dof limb that crosses the boundary between the column sets
struct EditedTree {
  static constexpr int NV = 19;
  static constexpr int dof_parentid[NV] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 10, 11, 12, 13, 14, 15, 16, 17};
};
#define MODEL EditedTree
#define NO_MADR
#endif
#include "duck_mcols.h"

int main() {
  using Md = MODEL;
  using MC = MCols<Md, 16>;
  std::printf("NV %d NC %d\nparent", Md::NV, MC::NC);
  for (int i = 0; i < Md::NV; i++) std::printf(" %d", Md::dof_parentid[i]);
  std::printf("\n");
  for (int s = 0; s < MC::NC; s++)
    for (int r = 0; r < Md::NV; r++)
      std::printf("row %d set %d d %u a %u z %u zero %d thresh %d depth %d\n", r, s, MC::dmask(r, s), MC::amask(r, s),
                  MC::zmask(r, s), (int)MC::zero_row(r, s), MC::thresh(r, s), MC::depth(r));
#ifndef NO_MADR
  for (int i = 0; i < Md::NV; i++) {
    std::printf("madr %d", i);
    for (int j = 0; j < Md::NV; j++) std::printf(" %d", Md::t_blob()[Md::B_MADR + Md::NV * i + j]);
    std::printf("\n");
  }
#endif
  return 0;
}
