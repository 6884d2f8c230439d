// The errors of the clip synth's two device functions (csrc/clip_synth_fn.h) against fp64, measured on the device they run on; the figures go
// into profiles/clip_synth_mi355x.txt and, rounded up, into tests/synth_emul.py.  A stand-alone program:
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -I nylon-amt_amd/csrc tools/synth_fn_error.hip -o synth_fn_error && ./synth_fn_error
//   S  over EVERY value u = (float)(int32)x * 2^-32 can take: x = m * 2^s with |m| < 2^24 (every int32 rounds to one of these), about 2^28
//      arguments -- exhaustive; the largest |S(u) - sin(2 pi u)| in absolute terms
//   E  over a dense grid y = -126 j / 2^24, j = 0 .. 2^24 (and the neighbouring float of each); the largest |E(y) / 2^y - 1|
// The reference is the host's fp64 sin / exp2 (libm), whose own error is some 2^-30 of the figures printed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "clip_synth_fn.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

__global__ void eval(const float* in, float* out, long n, int which) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = which ? synth_exp2(in[i]) : synth_sin_turns(in[i]);
}

static void run(const std::vector<float>& in, std::vector<float>& out, int which) {
  const long n = (long)in.size();
  float *din, *dout;
  out.resize(n);
  CHECK(hipMalloc(&din, n * 4));
  CHECK(hipMalloc(&dout, n * 4));
  CHECK(hipMemcpy(din, in.data(), n * 4, hipMemcpyHostToDevice));
  eval<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(din, dout, n, which);
  CHECK(hipGetLastError());
  CHECK(hipMemcpy(out.data(), dout, n * 4, hipMemcpyDeviceToHost));
  CHECK(hipFree(din));
  CHECK(hipFree(dout));
}

int main() {
  const double two_pi = 6.283185307179586476925286766559;
  std::vector<float> in, out;
  double worst_s = 0.0, at_s = 0.0;
  long count_s = 0;
  for (int s = 0; s <= 7; s++) {                       // x = m 2^s: s = 0 holds every |x| <= 2^24, s > 0 the floats of exponent 23 + s
    in.clear();
    const long m0 = s == 0 ? 0 : (1l << 23);
    for (long m = m0; m <= (1l << 24); m++) {
      const double x = ldexp((double)m, s);
      if (x > 2147483648.0) break;                     // (float)(int32) reaches 2^31 by rounding, and -2^31
      in.push_back((float)(x * 0x1p-32));
      in.push_back((float)(-x * 0x1p-32));
    }
    run(in, out, 0);
    for (size_t i = 0; i < in.size(); i++) {
      const double e = fabs((double)out[i] - sin(two_pi * (double)in[i]));
      if (e > worst_s) { worst_s = e; at_s = in[i]; }
    }
    count_s += (long)in.size();
  }
  printf("S = v_sin_f32 (turns): %ld arguments, largest |S(u) - sin(2 pi u)| = %.6e = 2^%.3f at u = %.9g\n", count_s, worst_s, log2(worst_s), at_s);
  in.clear();
  for (long j = 0; j <= (1l << 24); j++) {
    const float y = (float)(-126.0 * (double)j / 16777216.0);
    in.push_back(y);
    in.push_back(fmaxf(nextafterf(y, -200.f), -126.f));
  }
  run(in, out, 1);
  double worst_e = 0.0, at_e = 0.0;
  for (size_t i = 0; i < in.size(); i++) {
    const double e = fabs((double)out[i] / exp2((double)in[i]) - 1.0);
    if (e > worst_e) { worst_e = e; at_e = in[i]; }
  }
  printf("E = v_exp_f32: %zu arguments in [-126, 0], largest |E(y) / 2^y - 1| = %.6e = 2^%.3f at y = %.9g\n", in.size(), worst_e, log2(worst_e), at_e);
  return 0;
}
