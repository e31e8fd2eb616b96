// atan2 in double-double arithmetic, rounded once to float64: the correctly rounded value except where the true value lies within
// about 2^-40 ulp of a rounding boundary.  glibc's atan2 (what numpy's angle and OCaml's Float.atan2 call) is the correctly rounded
// value in that sense too, so the two agree to the last bit -- which the phase vocoder needs (effects.hip): its accumulator
// reaches 1e6 rad, where one float64 ulp is 2e-10, and an argument that differs in its last bit (2e-16) moves a later sum across a
// rounding boundary.  The device library's atan2 is accurate to an ulp or two, not to half of one.
//
// t = min(|x|, |y|) / max(|x|, |y|) as a double-double quotient; c = rint(64 t) / 64; r = (t - c) / (1 + t c), |r| <= 2^-7;
// atan t = atan c (table, double-double) + r + r^3 P(r^2), P to r^14; then the octant.  Zeros, infinities, NaNs and ratios
// near the ends of the exponent range go to the library function (exact constants and cases no spectrum holds).
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define SMX_DD_FN __device__ __forceinline__
#define SMX_DD_TABLE __device__ const
#else
#define SMX_DD_FN inline
#define SMX_DD_TABLE static const
#endif

namespace smx {
namespace dd {

#define SMX_DD_KPI_HI 0x1.921fb54442d18p+1
#define SMX_DD_KPI_LO 0x1.1a62633145c07p-53
#define SMX_DD_KPIO2_HI 0x1.921fb54442d18p+0
#define SMX_DD_KPIO2_LO 0x1.1a62633145c07p-54
#define SMX_DD_KTHIRD_HI 0x1.5555555555555p-2
#define SMX_DD_KTHIRD_LO 0x1.5555555555555p-56
#define SMX_DD_KFIFTH_HI 0x1.999999999999ap-3
#define SMX_DD_KFIFTH_LO -0x1.999999999999ap-57

// atan(i / 64), i = 0 .. 64: the float64 value and what it leaves of the exact one
SMX_DD_TABLE double kAtanTable[65][2] = {
  {0x0.0p+0, 0x0.0p+0},
  {0x1.fff555bbb729bp-7, -0x1.220c39d4dff50p-61},
  {0x1.ffd55bba97625p-6, -0x1.5ec431444912cp-60},
  {0x1.7fb818430da2ap-5, -0x1.86ef8f794f105p-63},
  {0x1.ff55bb72cfdeap-5, -0x1.c934d86d23f1dp-60},
  {0x1.3f59f0e7c559dp-4, 0x1.ac4ce285df847p-58},
  {0x1.7ee182602f10fp-4, -0x1.cfb654c0c3d98p-58},
  {0x1.be39ebe6f07c3p-4, 0x1.f7b8f29a05987p-58},
  {0x1.fd5ba9aac2f6ep-4, -0x1.cd37686760c17p-59},
  {0x1.1e1fafb043727p-3, -0x1.b485914dacf8cp-59},
  {0x1.3d6eee8c6626cp-3, 0x1.61a3b0ce9281bp-57},
  {0x1.5c9811e3ec26ap-3, -0x1.054ab2c010f3dp-58},
  {0x1.7b97b4bce5b02p-3, 0x1.347b0b4f881cap-58},
  {0x1.9a6a8e96c8626p-3, 0x1.cf601e7b4348ep-59},
  {0x1.b90d7529260a2p-3, 0x1.17b10d2e0e5abp-61},
  {0x1.d77d5df205736p-3, 0x1.c648d1534597ep-57},
  {0x1.f5b75f92c80ddp-3, 0x1.8ab6e3cf7afbdp-57},
  {0x1.09dc597d86362p-2, 0x1.62e47390cb865p-56},
  {0x1.18bf5a30bf178p-2, 0x1.30ca4748b1bf9p-57},
  {0x1.278372057ef46p-2, -0x1.077cdd36dfc81p-56},
  {0x1.362773707ebccp-2, -0x1.963a544b672d8p-57},
  {0x1.44aa436c2af0ap-2, -0x1.5d5e43c55b3bap-56},
  {0x1.530ad9951cd4ap-2, -0x1.2566480884082p-57},
  {0x1.614840309cfe2p-2, -0x1.a725715711f00p-56},
  {0x1.6f61941e4def1p-2, -0x1.c63aae6f6e918p-56},
  {0x1.7d5604b63b3f7p-2, 0x1.69c885c2b249ap-56},
  {0x1.8b24d394a1b25p-2, 0x1.b6d0ba3748fa8p-56},
  {0x1.98cd5454d6b18p-2, 0x1.9e6c988fd0a77p-56},
  {0x1.a64eec3cc23fdp-2, -0x1.24dec1b50b7ffp-56},
  {0x1.b3a911da65c6cp-2, 0x1.ae187b1ca5040p-56},
  {0x1.c0db4c94ec9f0p-2, -0x1.cc1ce70934c34p-56},
  {0x1.cde53432c1351p-2, -0x1.a2cfa4418f1adp-56},
  {0x1.dac670561bb4fp-2, 0x1.a2b7f222f65e2p-56},
  {0x1.e77eb7f175a34p-2, 0x1.0e53dc1bf3435p-56},
  {0x1.f40dd0b541418p-2, -0x1.a3992dc382a23p-57},
  {0x1.0039c73c1a40cp-1, -0x1.b32c949c9d593p-55},
  {0x1.0657e94db30d0p-1, -0x1.d5b495f6349e6p-56},
  {0x1.0c6145b5b43dap-1, 0x1.974fa13b5404fp-58},
  {0x1.1255d9bfbd2a9p-1, -0x1.2bdaee1c0ee35p-58},
  {0x1.1835a88be7c13p-1, 0x1.c621cec00c301p-55},
  {0x1.1e00babdefeb4p-1, -0x1.928df287a668fp-58},
  {0x1.23b71e2cc9e6ap-1, 0x1.c421c9f38224ep-57},
  {0x1.2958e59308e31p-1, -0x1.09e73b0c6c087p-56},
  {0x1.2ee628406cbcap-1, 0x1.c5d5e9ff0cf8dp-55},
  {0x1.345f01cce37bbp-1, 0x1.1021137c71102p-55},
  {0x1.39c391cd4171ap-1, -0x1.2304331d8bf46p-55},
  {0x1.3f13fb89e96f4p-1, 0x1.ecf8b492644f0p-56},
  {0x1.445065b795b56p-1, -0x1.f76d0163f79c8p-56},
  {0x1.4978fa3269ee1p-1, 0x1.2419a87f2a458p-56},
  {0x1.4e8de5bb6ec04p-1, 0x1.4a33dbeb3796cp-55},
  {0x1.538f57b89061fp-1, -0x1.1bb74abda520cp-55},
  {0x1.587d81f732fbbp-1, -0x1.5e5c9d8c5a950p-56},
  {0x1.5d58987169b18p-1, 0x1.0028e4bc5e7cap-57},
  {0x1.6220d115d7b8ep-1, -0x1.2b785350ee8c1p-57},
  {0x1.66d663923e087p-1, -0x1.6ea6febe8bbbap-56},
  {0x1.6b798920b3d99p-1, -0x1.a80386188c50ep-55},
  {0x1.700a7c5784634p-1, -0x1.8c34d25aadef6p-56},
  {0x1.748978fba8e0fp-1, 0x1.7b2a6165884a1p-59},
  {0x1.78f6bbd5d315ep-1, 0x1.406a089803740p-55},
  {0x1.7d528289fa093p-1, 0x1.560821e2f3aa9p-55},
  {0x1.819d0b7158a4dp-1, -0x1.bf76229d3b917p-56},
  {0x1.85d69576cc2c5p-1, 0x1.6b66e7fc8b8c3p-57},
  {0x1.89ff5ff57f1f8p-1, -0x1.55b9a5e177a1bp-55},
  {0x1.8e17aa99cc05ep-1, -0x1.ec182ab042f61p-56},
  {0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55},
};

struct Pair {
  double hi, lo;
};

SMX_DD_FN Pair fast_two_sum(double a, double b) {   // |a| >= |b|
  const double s = a + b;
  return {s, b - (s - a)};
}
SMX_DD_FN Pair two_sum(double a, double b) {
  const double s = a + b, v = s - a;
  return {s, (a - (s - v)) + (b - v)};
}
SMX_DD_FN Pair two_prod(double a, double b) {
  const double p = a * b;
  return {p, fma(a, b, -p)};
}
SMX_DD_FN Pair add(Pair a, Pair b) {
  Pair s = two_sum(a.hi, b.hi);
  const Pair t = two_sum(a.lo, b.lo);
  s.lo += t.hi;
  s = fast_two_sum(s.hi, s.lo);
  s.lo += t.lo;
  return fast_two_sum(s.hi, s.lo);
}
SMX_DD_FN Pair neg(Pair a) { return {-a.hi, -a.lo}; }
SMX_DD_FN Pair mul(Pair a, Pair b) {
  Pair p = two_prod(a.hi, b.hi);
  p.lo += (a.hi * b.lo) + (a.lo * b.hi);
  return fast_two_sum(p.hi, p.lo);
}
SMX_DD_FN Pair div(Pair a, Pair b) {
  const double q1 = a.hi / b.hi;
  const Pair r1 = add(a, neg(mul(b, Pair{q1, 0.0})));
  const double q2 = r1.hi / b.hi;
  const Pair r2 = add(r1, neg(mul(b, Pair{q2, 0.0})));
  const double q3 = r2.hi / b.hi;
  const Pair q = fast_two_sum(q1, q2);
  return add(q, Pair{q3, 0.0});
}

SMX_DD_FN double atan2_rounded(double y, double x) {
  const double ax = fabs(x), ay = fabs(y);
  const double big = ax > ay ? ax : ay, small = ax > ay ? ay : ax;
  if (!(big < 0x1p+500) || !(small > 0x1p-500) || !(small > big * 0x1p-400)) return atan2(y, x);
  // t = small / big: the quotient, the exact remainder by one fused multiply-add, and its quotient
  const double q1 = small / big;
  const double q2 = fma(-q1, big, small) / big;
  const Pair t = fast_two_sum(q1, q2);
  const int i = (int)rint(t.hi * 64.0);
  const double c = (double)i * 0.015625;
  Pair tc = two_prod(t.hi, c);
  tc.lo += t.lo * c;
  const Pair r = div(add(t, Pair{-c, 0.0}), add(Pair{1.0, 0.0}, fast_two_sum(tc.hi, tc.lo)));
  const Pair s = mul(r, r);
  const double z = s.hi;
  const double tail = (z * z) * (-1.0 / 7.0 + z * (1.0 / 9.0 + z * (-1.0 / 11.0 + z * (1.0 / 13.0 - z * (1.0 / 15.0)))));
  const Pair p = add(add(Pair{-SMX_DD_KTHIRD_HI, -SMX_DD_KTHIRD_LO}, mul(s, Pair{SMX_DD_KFIFTH_HI, SMX_DD_KFIFTH_LO})), Pair{tail, 0.0});
  Pair a = add(Pair{kAtanTable[i][0], kAtanTable[i][1]}, add(r, mul(mul(r, s), p)));
  if (ay > ax) a = add(Pair{SMX_DD_KPIO2_HI, SMX_DD_KPIO2_LO}, neg(a));
  if (x < 0.0) a = add(Pair{SMX_DD_KPI_HI, SMX_DD_KPI_LO}, neg(a));
  return y < 0.0 ? -a.hi : a.hi;
}

}  // namespace dd
}  // namespace smx
