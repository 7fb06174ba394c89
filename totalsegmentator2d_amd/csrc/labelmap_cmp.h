// The comparator of the label-map export (kernels_labelmap.h): numpy's argmax on float32, one step of it.  numpy walks the heads in
// index order and replaces its running maximum when `!(v <= best)`, and stops at the first NaN it has taken - so the first index of the
// maximum wins, +0 and -0 are equal (neither replaces the other), a NaN beats every number and the first NaN stays.
// Its own header, host and device: tests/test_labelmap_cpu.py compiles it as plain C++ and exhausts it against np.argmax.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TS2D_LM_HD __host__ __device__ __forceinline__
#else
#define TS2D_LM_HD inline
#endif

namespace ts2d {

// does head value `v` replace the running maximum `best` of the heads before it?
TS2D_LM_HD bool lm_replaces(float v, float best) { return best == best && !(v <= best); }

}  // namespace ts2d
