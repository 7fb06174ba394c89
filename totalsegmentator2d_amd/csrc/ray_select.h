// The selection behind the median projection (kernels_project_modes.h): order-preserving unsigned keys of the five volume types and the
// k-th smallest of a ray by MSB-first bitwise selection on them.  Their own header, host and device: tests/test_projection_modes_cpu.py
// compiles it as plain C++ and holds rs_select_kth against np.sort(ray)[k] for every key type.
//
// Keys.  rs_key maps a sample to an unsigned integer of its own width so that a < b  <=>  key(a) < key(b): unsigned types are their own
// key, signed ones have the sign bit flipped, a float has all bits flipped when negative and the sign bit flipped otherwise (so -0.0 sorts
// right below +0.0 and the subnormals between the zeros and the normals; a NaN has no place in the order: the callers keep non-finite
// volumes off this path).  rs_unkey is the inverse.
//
// Selection.  The key of the k-th smallest (k from 0) is built from its top bit down.  With the bits above b decided (`prefix`), a pass
// counts the candidates - the keys that agree with the prefix on those bits - whose bit b is clear.  If k is below that count the answer
// is among them and bit b stays clear; otherwise the count is taken off k and bit b is set.  After the last bit `prefix` is a key that
// occurs in the ray at sorted position k.  Integers only; every trip count is fixed (key bits x n), nothing depends on the data.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TS2D_RS_HD __host__ __device__ __forceinline__
#else
#define TS2D_RS_HD inline
#endif

namespace ts2d {

template <typename T> struct RsKey;
template <> struct RsKey<uint8_t>  { typedef uint8_t  type; static constexpr int bits = 8; };
template <> struct RsKey<int16_t>  { typedef uint16_t type; static constexpr int bits = 16; };
template <> struct RsKey<uint16_t> { typedef uint16_t type; static constexpr int bits = 16; };
template <> struct RsKey<int32_t>  { typedef uint32_t type; static constexpr int bits = 32; };
template <> struct RsKey<float>    { typedef uint32_t type; static constexpr int bits = 32; };

TS2D_RS_HD uint8_t  rs_key(uint8_t v)  { return v; }
TS2D_RS_HD uint16_t rs_key(uint16_t v) { return v; }
TS2D_RS_HD uint16_t rs_key(int16_t v)  { return (uint16_t)((uint16_t)v ^ 0x8000u); }
TS2D_RS_HD uint32_t rs_key(int32_t v)  { return (uint32_t)v ^ 0x80000000u; }
TS2D_RS_HD uint32_t rs_key(float v) {
    uint32_t u;
    memcpy(&u, &v, sizeof(u));
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <typename T> TS2D_RS_HD T rs_unkey(typename RsKey<T>::type k);
template <> TS2D_RS_HD uint8_t  rs_unkey<uint8_t>(uint8_t k)   { return k; }
template <> TS2D_RS_HD uint16_t rs_unkey<uint16_t>(uint16_t k) { return k; }
template <> TS2D_RS_HD int16_t  rs_unkey<int16_t>(uint16_t k)  { return (int16_t)(uint16_t)(k ^ 0x8000u); }
template <> TS2D_RS_HD int32_t  rs_unkey<int32_t>(uint32_t k)  { return (int32_t)(k ^ 0x80000000u); }
template <> TS2D_RS_HD float    rs_unkey<float>(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float v;
    memcpy(&v, &u, sizeof(v));
    return v;
}

// Is `key` a candidate with bit b clear?  sel = the decided bits above b together with bit b itself; prefix has bit b (and all below) clear.
TS2D_RS_HD int rs_counts(uint32_t key, uint32_t sel, uint32_t prefix) { return (key & sel) == prefix ? 1 : 0; }

// One decision: `clear` candidates have bit `bit` clear.  Keeps k and the prefix, or takes the count off k and sets the bit.
TS2D_RS_HD void rs_decide(int clear, uint32_t bit, int* k, uint32_t* prefix) {
    if (*k >= clear) { *k -= clear; *prefix |= bit; }
}

// The key at sorted position k (0 <= k < n) of keys[0], keys[stride], ..., keys[(n - 1) stride]: KEY_BITS passes of n reads each.
template <typename K, int KEY_BITS>
TS2D_RS_HD K rs_select_kth(const K* keys, int n, long long stride, int k) {
    uint32_t prefix = 0, sel = 0;
    for (int b = KEY_BITS - 1; b >= 0; --b) {
        const uint32_t bit = 1u << b;
        sel |= bit;
        int clear = 0;
        for (int i = 0; i < n; ++i) clear += rs_counts((uint32_t)keys[i * stride], sel, prefix);
        rs_decide(clear, bit, &k, &prefix);
    }
    return (K)prefix;
}

// The same over samples of type T (the key is taken at every read): the variant that re-reads the ray once per key bit.
template <typename T>
TS2D_RS_HD T rs_select_kth_samples(const T* ray, int n, long long stride, int k) {
    uint32_t prefix = 0, sel = 0;
    for (int b = RsKey<T>::bits - 1; b >= 0; --b) {
        const uint32_t bit = 1u << b;
        sel |= bit;
        int clear = 0;
        for (int i = 0; i < n; ++i) clear += rs_counts((uint32_t)rs_key(ray[i * stride]), sel, prefix);
        rs_decide(clear, bit, &k, &prefix);
    }
    return rs_unkey<T>((typename RsKey<T>::type)prefix);
}

}  // namespace ts2d
