// Which instantiation of k_msp_leaf (rfx_msp.hip) a launch takes.  Plain C++, no device code: msp_leaf() asks it, and
// tests/host/leaf_variant_harness.cpp prints it for the host suite.
#pragma once

// The k the kernel is compiled for (template parameter KC; the single-segment form ONE goes with it), or 0: the generic
// kernel with k, the segment tables and force_mixed as arguments.  Specialised: RUFUS's default k = 25 and the 31 of the
// tumor / normal configuration, when the launch has ONE segment (the trio route: part2_multi puts all blocks into one
// stream) and neither test knob is set -- RFX_LEAF_FORCE_MIXED (the recount route, which the specialised kernels do not
// carry) or RFX_LEAF_GENERIC (A/B and bisecting).
inline int msp_leaf_kc(int k, int nseg, bool force_mixed, bool force_generic) {
  if (nseg != 1 || force_mixed || force_generic) return 0;
  return k == 25 || k == 31 ? k : 0;
}
