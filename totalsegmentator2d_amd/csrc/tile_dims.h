// The workgroup tile every kernel of kernels*.h is written against.  Its own header because the host-side dispatch (dispatch.cpp, which is
// compiled without an offload pass and includes no kernel) tests an op's eligibility against the same two numbers.
#pragma once

namespace ts2d {

constexpr int kBlock = 256;   // threads per workgroup (4 waves, one per SIMD)
constexpr int kBM = 256;      // output pixels per workgroup tile
// conv3x3s2_v2 (kernels_s2v2.h): bytes of one LDS plane of its patch (17 rows x 66 slots + 2 of padding, 16 bytes each) and the LDS a workgroup may
// ask for - what decides whether a column tile's weights stay resident beside the patch
constexpr int kS2PlaneBytes = (17 * 66 + 2) * 16;
constexpr int kS2LdsMax = 160 * 1024;

}  // namespace ts2d
