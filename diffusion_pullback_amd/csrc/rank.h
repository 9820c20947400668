// The descending rank order of the geometry kernels and the NaN-propagating maximum of the convergence figures: plain C++ with no HIP include, so the
// same text compiles for the device (geom.h) and in a host program (tests/host/rank_order_host.cpp) that checks the index property on the CPU.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DPB_HD __host__ __device__
#else
#define DPB_HD
#endif

namespace dpb {

// the descending order of the rank counting: a NaN sorts before every number and ties go by index, so the ranks are a permutation whatever the values
DPB_HD inline bool sorts_before(double other, double mine, bool other_first) {
  const bool on = other != other, mn = mine != mine;
  if (on || mn) return on && (!mn || other_first);
  return other > mine || (other == mine && other_first);
}

// the rank of v[t] among v[0 .. k-1] in that order: in [0, k) and distinct for distinct t, for any values.  Without a NaN it is the plain comparison
// (v[e] > v[t], ties by index) -- which alone gives every NaN rank 0 and leaves the other slots of an `order[rank] = t` scatter unwritten.
DPB_HD inline int rank_desc(const double* v, int k, int t) {
  int rank = 0;
  const double mine = v[t];
  for (int e = 0; e < k; ++e) rank += sorts_before(v[e], mine, e < t) ? 1 : 0;
  return rank;
}

// max(a, b) that keeps a NaN operand (fmax / fmaxf drop it).  On numbers it is fmax (the callers' operands are never -0)
template <typename T>
DPB_HD inline T max_nan(T a, T b) { return (b > a || b != b) ? b : a; }

}  // namespace dpb
