// Prints the dispatch rule of k_msp_leaf (rufus_amd/csrc/rfx_leaf_variant.h, the function msp_leaf() asks) as a table:
// one line "k nseg force_mixed force_generic kc" per combination, for tests/test_leaf_variant_host.py.  TEST INFRASTRUCTURE.
#include <cstdio>

#include "../../rufus_amd/csrc/rfx_leaf_variant.h"

int main() {
  for (int k = 15; k <= 32; ++k)
    for (int nseg = 1; nseg <= 4; ++nseg)
      for (int fm = 0; fm < 2; ++fm)
        for (int fg = 0; fg < 2; ++fg) printf("%d %d %d %d %d\n", k, nseg, fm, fg, msp_leaf_kc(k, nseg, fm != 0, fg != 0));
  return 0;
}
