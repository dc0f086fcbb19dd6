// pcp_eigen33_selftest.hpp -- one lane of pcp_selftest_eigen33: the device functions of pcp_eigen33.hpp on a caller's input.
// Included by the units whose compilation of the solver the self-test stands for, BEHIND pcp_eigen33.hpp and under the
// floating-point contraction that unit's own caller of smallest_eigenpair is compiled with: pcp_normals.hip (none; form 0,
// which is also how pcp_crack_width.hip and pcp_crack_direction.hip build it) and pcp_mls.hip (contract(fast), as k_mls_fit;
// form 1).  Lane i < n solves matrix i, lane i < m maps argument i; nothing is reduced, NaNs and infinities go out as they are.
#pragma once

#include <cstdint>

#include "pcp_eigen33.hpp"

namespace pcp {

struct Eigen33SelftestArgs {
  const double *mat;  // 6 n: xx xy xz yy yz zz
  double *ev;         // n
  double *vec;        // 3 n
  int64_t n;
  const double *arg;  // m
  double *rcp;        // m
  double *rsqrt;      // m
  int64_t m;
};

__device__ __forceinline__ void eigen33_selftest_lane(const Eigen33SelftestArgs &a, int64_t i) {
  if (i < a.n) {
    double M[6], ev, v[3];
    for (int k = 0; k < 6; ++k) M[k] = a.mat[6 * i + k];
    smallest_eigenpair(M, ev, v);
    a.ev[i] = ev;
    for (int k = 0; k < 3; ++k) a.vec[3 * i + k] = v[k];
  }
  if (i < a.m) {
    const double x = a.arg[i];
    a.rcp[i] = mls_rcp(x);
    a.rsqrt[i] = mls_rsqrt(x);
  }
}

// the launch of form 1 (pcp_mls.hip); form 0's stands beside the entry point in pcp_normals.hip
void selftest_eigen33_launch_contracted(const Eigen33SelftestArgs &a, hipStream_t stream);

}  // namespace pcp
