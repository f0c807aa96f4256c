// What does v_cvt_scalef32_pk_fp4_f32 do at ties, beyond 6, with signed zeros, and with its scale operand?
// (csrc/mxfp4_quantize.hip relies on: scale 1.0 leaves the value alone; round to nearest, ties to even; 6 stays 6.)
//   hipcc --offload-arch=gfx950 tools/probe_cvt_fp4.hip -o probe_cvt_fp4 && ./probe_cvt_fp4
// Prints every probed value with the code the instruction gave and the code a compare ladder gives, then the number
// of disagreements over a sweep of [-8, 8] in steps of 1/64 at scale 1.0, then 4.0 converted at scales 8 and 1/8.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

__global__ void k(const float* in, const float* scale, unsigned* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  // the value in the low nibble, 1.0 (code 2) in the high one; the other three bytes keep the old word
  if (i < n) out[i] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0xAABBCC00u, in[i], 1.0f, scale[i], 0);
}

// e2m1, nearest with ties to even, saturating: magnitudes 0 .5 1 1.5 2 3 4 6 are codes 0 .. 7, bit 3 is the sign
static unsigned ladder(float x) {
  const float a = x < 0 ? -x : x;
  const unsigned c = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
  return c | (__builtin_signbit(x) ? 8u : 0u);
}

int main() {
  std::vector<float> vals = {0.f, -0.f, 0.125f, 0.25f, 0.2500001f, 0.5f, 0.75f, 1.f, 1.25f, 1.5f, 1.75f, 2.f, 2.5f, 3.f, 3.5f,
                             4.f, 5.f, 5.0000005f, 6.f, -0.25f, -0.75f, -1.25f, -1.75f, -2.5f, -3.5f, -5.f, -6.f, 6.5f, 7.f, 100.f,
                             -100.f, 1e-30f};
  const int named = (int)vals.size();
  for (int i = -512; i <= 512; ++i) vals.push_back(i / 64.f);
  std::vector<float> scales(vals.size(), 1.0f);
  vals.push_back(4.f); scales.push_back(8.f);
  vals.push_back(4.f); scales.push_back(0.125f);
  const int n = (int)vals.size();
  float *d_in, *d_scale; unsigned* d_out;
  std::vector<unsigned> h(n);
  if (hipMalloc(&d_in, n * 4) != hipSuccess || hipMalloc(&d_scale, n * 4) != hipSuccess || hipMalloc(&d_out, n * 4) != hipSuccess) return 1;
  hipMemcpy(d_in, vals.data(), n * 4, hipMemcpyHostToDevice);
  hipMemcpy(d_scale, scales.data(), n * 4, hipMemcpyHostToDevice);
  k<<<(n + 255) / 256, 256>>>(d_in, d_scale, d_out, n);
  if (hipMemcpy(h.data(), d_out, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  for (int i = 0; i < named; ++i)
    printf("%14.8g -> word %08x  code %x  ladder %x%s\n", vals[i], h[i], h[i] & 15, ladder(vals[i]),
           (h[i] & 15) == ladder(vals[i]) ? "" : "  DIFFERS");
  int differ = 0, differ_beyond_sign_of_zero = 0, words_off = 0;
  for (int i = named; i < n - 2; ++i) {
    const unsigned got = h[i] & 15, want = ladder(vals[i]);
    differ += got != want;
    differ_beyond_sign_of_zero += got != want && ((got | want) & 7) != 0;
    words_off += (h[i] >> 4) != 0xAABBCC2u;
  }
  printf("sweep [-8, 8] step 1/64: %d of %d differ from the ladder, %d of them other than in the sign of a zero; "
         "%d words with the high nibble or the kept bytes off\n", differ, n - 2 - named, differ_beyond_sign_of_zero, words_off);
  printf("4.0 at scale 8     -> code %x (1 = .5: the value is divided by the scale; 7 = 6: multiplied)\n", h[n - 2] & 15);
  printf("4.0 at scale 0.125 -> code %x (7 = 6: divided; 1 = .5: multiplied)\n", h[n - 1] & 15);
  return 0;
}
