// Host build of the kernel and launcher of ganslate_amd/csrc/visgrid.hip: the HIP keywords are defined away, a launch is a
// serial loop over the grid, and visgrid_body.inc is that file without its common.hpp include (written by
// tests/test_visgrid_host_cpu.py). Every buffer has exactly the size the C ABI states, so AddressSanitizer sees any access
// the kernel makes outside it; the image is compared byte for byte with a plain loop.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <cstdarg>
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 blockIdx, threadIdx;
struct alignas(16) float4 { float x, y, z, w; };
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
typedef void* hipStream_t; typedef int hipError_t;
#define hipSuccess 0
static int hipGetLastError() { return 0; }
static char g_err[512];
static void gs_set_error(const char* fmt, ...) { va_list a; va_start(a, fmt); vsnprintf(g_err, sizeof g_err, fmt, a); va_end(a); }
#define GS_CHECK_HIP(x) do { if ((x) != hipSuccess) return 1; } while (0)
#define GS_REQUIRE(cond, ...) do { if (!(cond)) { gs_set_error(__VA_ARGS__); return 2; } } while (0)
#define hipLaunchKernelGGL(k, grid, block, shm, st, ...) do { dim3 g_ = (grid), b_ = (block); \
  for (unsigned z_ = 0; z_ < g_.z; ++z_) for (unsigned y_ = 0; y_ < g_.y; ++y_) for (unsigned x_ = 0; x_ < g_.x; ++x_) \
  for (unsigned t_ = 0; t_ < b_.x; ++t_) { blockIdx = dim3(x_, y_, z_); threadIdx = dim3(t_, 0, 0); k(__VA_ARGS__); } } while (0)
#include "visgrid_body.inc"

// the separate ops, each result stored to a float before the next
static uint8_t ref_byte(float v) {
  volatile float t = v + 1.0f;
  t = t / 2.0f;
  t = t * 255.0f;
  t = t + 0.5f;
  float u = t;
  if (std::isnan(u)) return 0;
  if (u < 0.0f) u = 0.0f;
  if (u > 255.0f) u = 255.0f;
  return (uint8_t)(int)u;
}

static std::vector<float> g_values;      // the threshold neighbours and the specials
static void fill_values() {
  for (int k = 1; k <= 255; ++k) {
    float x = (float)(2.0 * (k - 0.5) / 255.0 - 1.0);
    float lo = x, hi = x;
    std::vector<float> below;
    for (int i = 0; i < 8; ++i) { lo = std::nextafterf(lo, -INFINITY); below.push_back(lo); }
    for (int i = 7; i >= 0; --i) g_values.push_back(below[i]);
    g_values.push_back(x);
    for (int i = 0; i < 8; ++i) { hi = std::nextafterf(hi, INFINITY); g_values.push_back(hi); }
  }
  const float special[] = {-0.0f, 1.0f, -1.0f, 1.5f, -1.5f, INFINITY, -INFINITY, NAN};
  for (float s : special) g_values.push_back(s);
  for (int i = 0; i < 257; ++i) g_values.push_back(((float)rand() / RAND_MAX - 0.5f) * 6.0f);
}

struct Visual { int ctot, c0, c, tensor, misalign; };    // tensor: visuals with the same number share one buffer

static int run_case(const char* what, int N, int n, int D, int H, int W, int slice, std::vector<Visual> vis, int out_misalign) {
  static size_t walk = 0;
  const int K = (int)vis.size();
  const size_t vol = (size_t)D * H * W;
  std::vector<float*> base(K, nullptr), data(K, nullptr);
  for (int k = 0; k < K; ++k) {
    if (vis[k].tensor < k) { base[k] = nullptr; data[k] = data[vis[k].tensor]; continue; }
    const size_t count = (size_t)N * vis[k].ctot * vol;
    void* p; if (posix_memalign(&p, 64, (count + vis[k].misalign) * 4)) abort();    // exact size: ASan sees any overrun
    base[k] = (float*)p; data[k] = base[k] + vis[k].misalign;
    for (size_t i = 0; i < count; ++i) data[k][i] = g_values[walk++ % g_values.size()];
  }
  const int Dout = slice < 0 ? D : 1, rows = Dout * H;
  const size_t bytes = (size_t)n * rows * K * W * 3;
  uint8_t* obase = (uint8_t*)malloc(bytes + out_misalign);
  uint8_t* out = obase + out_misalign;
  memset(out, 0xA5, bytes);
  std::vector<const float*> src(K); std::vector<int32_t> ctot(K), c0(K), c(K);
  for (int k = 0; k < K; ++k) { src[k] = data[k]; ctot[k] = vis[k].ctot; c0[k] = vis[k].c0; c[k] = vis[k].c; }
  int bad = 0;
  if (gs_visuals_grid_u8(src.data(), ctot.data(), c0.data(), c.data(), K, n, N, D, H, W, slice, out, nullptr)) {
    printf("%s: rc: %s\n", what, g_err); return 1;
  }
  for (int s = 0; s < n; ++s) for (int dz = 0; dz < Dout; ++dz) for (int y = 0; y < H; ++y) for (int k = 0; k < K; ++k)
    for (int x = 0; x < W; ++x) for (int ch = 0; ch < 3; ++ch) {
      const int z = slice < 0 ? dz : slice;
      const int sc = vis[k].c0 + (vis[k].c == 3 ? ch : 0);
      const float v = data[k][(((size_t)s * vis[k].ctot + sc) * D + z) * H * W + (size_t)y * W + x];
      const uint8_t want = ref_byte(v);
      const uint8_t got = out[(((size_t)s * rows + dz * H + y) * ((size_t)K * W) + (size_t)k * W + x) * 3 + ch];
      if (want != got) { if (bad < 5) printf("  %s: s%d z%d y%d k%d x%d ch%d v=%a want %d got %d\n", what, s, z, y, k, x, ch, v, want, got); ++bad; }
    }
  printf("%s N%d n%d %dx%dx%d slice %d K%d: grid=%zu bytes %s\n", what, N, n, D, H, W, slice, K, bytes, bad ? "FAIL" : "ok");
  for (int k = 0; k < K; ++k) free(base[k]);
  free(obase);
  return bad;
}

static int expect_rejected(const char* what, int rc) {
  printf("%s: %s\n", what, rc ? "rejected" : "ACCEPTED (FAIL)");
  return rc == 0;
}

int main() {
  fill_values();
  int bad = 0;
  // one walk through all of g_values: every byte threshold with its neighbours
  bad += run_case("thresholds", 1, 1, 1, 72, 64, -1, {{1, 0, 1, 0, 0}}, 0);
  bad += run_case("2d vector", 2, 2, 1, 5, 8, -1, {{3, 0, 3, 0, 0}, {1, 0, 1, 1, 0}, {3, 0, 3, 2, 0}}, 0);
  bad += run_case("2d scalar", 2, 2, 1, 5, 7, -1, {{3, 0, 3, 0, 0}, {1, 0, 1, 1, 0}, {3, 0, 3, 2, 0}}, 0);
  bad += run_case("misaligned source", 2, 2, 1, 5, 8, -1, {{3, 0, 3, 0, 1}, {1, 0, 1, 1, 0}, {3, 0, 3, 2, 0}}, 0);
  bad += run_case("misaligned output", 2, 2, 1, 5, 8, -1, {{3, 0, 3, 0, 0}, {1, 0, 1, 1, 0}}, 1);
  bad += run_case("single example", 3, 1, 1, 5, 8, -1, {{3, 0, 3, 0, 0}, {1, 0, 1, 1, 0}}, 0);
  bad += run_case("3d stacked", 2, 2, 3, 4, 6, -1, {{1, 0, 1, 0, 0}, {1, 0, 1, 1, 0}, {1, 0, 1, 2, 0}}, 0);
  bad += run_case("3d stacked vector", 2, 2, 3, 4, 8, -1, {{1, 0, 1, 0, 0}, {3, 0, 3, 1, 0}}, 0);
  bad += run_case("3d mid slice D3", 2, 2, 3, 4, 6, 1, {{1, 0, 1, 0, 0}, {1, 0, 1, 1, 0}, {1, 0, 1, 2, 0}}, 0);
  bad += run_case("3d mid slice D4", 2, 2, 4, 4, 6, 2, {{1, 0, 1, 0, 0}, {1, 0, 1, 1, 0}, {1, 0, 1, 2, 0}}, 0);
  bad += run_case("modality split", 2, 2, 1, 5, 8, -1, {{4, 0, 1, 0, 0}, {4, 1, 3, 0, 0}, {1, 0, 1, 2, 0}}, 0);
  bad += run_case("modality split 3d", 1, 1, 2, 3, 5, -1, {{4, 0, 1, 0, 0}, {4, 1, 3, 0, 0}, {1, 0, 1, 2, 0}}, 0);
  { std::vector<Visual> v; for (int k = 0; k < 16; ++k) v.push_back({1, 0, 1, k, 0});
    bad += run_case("16 visuals", 1, 1, 1, 2, 2, -1, v, 0); }
  bad += run_case("more than one block", 1, 1, 2, 40, 36, -1, {{3, 0, 3, 0, 0}, {1, 0, 1, 1, 0}}, 0);
  // what the launcher must refuse before it touches anything
  float one = 0.f; const float* s17[17]; int32_t a17[17], z17[17];
  for (int k = 0; k < 17; ++k) { s17[k] = &one; a17[k] = 1; z17[k] = 0; }
  uint8_t px[3];
  bad += expect_rejected("17 visuals", gs_visuals_grid_u8(s17, a17, z17, a17, 17, 1, 1, 1, 1, 1, -1, px, nullptr));
  int32_t two = 2, zero = 0, one_i = 1, three = 3;
  bad += expect_rejected("2 channels", gs_visuals_grid_u8(s17, &two, &zero, &two, 1, 1, 1, 1, 1, 1, -1, px, nullptr));
  bad += expect_rejected("channels past the tensor", gs_visuals_grid_u8(s17, &two, &zero, &three, 1, 1, 1, 1, 1, 1, -1, px, nullptr));
  bad += expect_rejected("n > N", gs_visuals_grid_u8(s17, &one_i, &zero, &one_i, 1, 2, 1, 1, 1, 1, -1, px, nullptr));
  bad += expect_rejected("slice == D", gs_visuals_grid_u8(s17, &one_i, &zero, &one_i, 1, 1, 1, 1, 1, 1, 1, px, nullptr));
  bad += expect_rejected("H * W >= 2^31", gs_visuals_grid_u8(s17, &one_i, &zero, &one_i, 1, 1, 1, 1, 65536, 32768, -1, px, nullptr));
  bad += expect_rejected("D > 65535", gs_visuals_grid_u8(s17, &one_i, &zero, &one_i, 1, 1, 1, 65536, 1, 1, -1, px, nullptr));
  printf(bad ? "FAILED\n" : "ALL OK\n");
  return bad != 0;
}
