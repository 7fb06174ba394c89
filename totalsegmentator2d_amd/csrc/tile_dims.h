// The workgroup tile every kernel of kernels*.h is written against.  Its own header because the host-side dispatch (dispatch.cpp, which is
// compiled without an offload pass and includes no kernel) tests an op's eligibility against the same two numbers.
#pragma once

namespace ts2d {

constexpr int kBlock = 256;   // threads per workgroup (4 waves, one per SIMD)
constexpr int kBM = 256;      // output pixels per workgroup tile

}  // namespace ts2d
