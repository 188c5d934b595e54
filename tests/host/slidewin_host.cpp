// Host build of the kernels and launchers of ganslate_amd/csrc/slidewin.hip: the HIP keywords are defined away, a launch is
// a serial loop over the grid, and slidewin_body.inc is that file without its common.hpp include (written by
// tests/test_sliding_window_host_cpu.py). Every buffer has exactly the size the C ABI states, so AddressSanitizer sees any
// access a kernel makes outside it; results are compared bit for bit with a padded copy and a sequential loop.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <climits>
#include <cmath>
#include <vector>
#include <algorithm>
#include <cstdarg>
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 blockIdx, threadIdx;
struct alignas(16) int4 { int x, y, z, w; };
struct alignas(16) float4 { float x, y, z, w; };
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
using std::min; using std::max;
typedef void* hipStream_t; typedef int hipError_t;
#define hipSuccess 0
static int hipGetLastError() { return 0; }
static const char* hipGetErrorString(int) { return ""; }
static char g_err[512];
static void gs_set_error(const char* fmt, ...) { va_list a; va_start(a, fmt); vsnprintf(g_err, sizeof g_err, fmt, a); va_end(a); }
#define GS_CHECK_HIP(x) do { if ((x) != hipSuccess) return 1; } while (0)
#define GS_REQUIRE(cond, ...) do { if (!(cond)) { gs_set_error(__VA_ARGS__); return 2; } } while (0)
static inline float __fadd_rn(float a, float b) { return a + b; }
static inline float __fdiv_rn(float a, float b) { return a / b; }
#define hipLaunchKernelGGL(k, grid, block, shm, st, ...) do { dim3 g_ = (grid), b_ = (block); \
  for (unsigned z_ = 0; z_ < g_.z; ++z_) for (unsigned y_ = 0; y_ < g_.y; ++y_) for (unsigned x_ = 0; x_ < g_.x; ++x_) \
  for (unsigned t_ = 0; t_ < b_.x; ++t_) { blockIdx = dim3(x_, y_, z_); threadIdx = dim3(t_, 0, 0); k(__VA_ARGS__); } } while (0)
#include "slidewin_body.inc"

static std::vector<std::vector<int>> starts_axis(int s, int r, double ov) {
  int interval = r == s ? r : std::max((int)(r * (1 - ov)), 1);
  int num = (int)std::ceil((double)(s - r) / interval) + 1;
  std::vector<std::vector<int>> o; for (int k = 0; k < num; ++k) o.push_back({std::min(k * interval, s - r)}); return o;
}
static float* amalloc(size_t n) { void* p; if (posix_memalign(&p, 64, std::max<size_t>(n, 1) * 4)) abort(); return (float*)p; }

static int run_case(int B, int C, int Co, int D, int H, int W, int rd, int rh, int rw, double ov, int sw, int misalign) {
  int roi[3] = {rd, rh, rw}, sz0[3] = {D, H, W}, P[3], pb[3];
  for (int k = 0; k < 3; ++k) { P[k] = std::max(sz0[k], roi[k]); pb[k] = (P[k] - sz0[k]) / 2; }
  std::vector<int> rows;
  for (auto& z : starts_axis(P[0], rd, ov)) for (auto& y : starts_axis(P[1], rh, ov)) for (auto& x : starts_axis(P[2], rw, ov))
    for (int b = 0; b < B; ++b) { rows.push_back(b); rows.push_back(z[0]); rows.push_back(y[0]); rows.push_back(x[0]); }
  int n = rows.size() / 4;
  int* table; { void* p; posix_memalign(&p, 64, n * 16); table = (int*)p; memcpy(table, rows.data(), n * 16); }
  size_t V0 = (size_t)D * H * W, VP = (size_t)P[0] * P[1] * P[2], R = (size_t)rd * rh * rw;
  float* in = amalloc(B * C * V0 + misalign) + misalign;     // exact-size buffers: ASan sees any overrun
  for (size_t i = 0; i < B * C * V0; ++i) in[i] = (float)rand() / RAND_MAX * 2 - 1;
  float* imap = amalloc(R); for (size_t i = 0; i < R; ++i) imap[i] = 0.001f + (float)rand() / RAND_MAX;
  float cval = -1.f;
  // reference: padded copy, sequential loop
  std::vector<float> pad(B * C * VP, cval), racc(B * Co * VP, 0.f), rcnt(B * VP, 0.f), want(B * Co * V0);
  for (int b = 0; b < B; ++b) for (int c = 0; c < C; ++c) for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x)
    pad[((size_t)(b * C + c) * P[0] + z + pb[0]) * P[1] * P[2] + (size_t)(y + pb[1]) * P[2] + x + pb[2]] = in[((size_t)(b * C + c) * D + z) * H * W + (size_t)y * W + x];
  float* acc = amalloc(B * Co * VP); memset(acc, 0, B * Co * VP * 4);
  int bad = 0;
  for (int g0 = 0; g0 < n; g0 += sw) {
    int m = std::min(sw, n - g0);
    float* win = amalloc(m * C * R); for (size_t i = 0; i < m * C * R; ++i) win[i] = NAN;
    if (gs_sw_gather(in, B, C, D, H, W, table + 4 * g0, m, roi, pb, cval, win, nullptr)) { printf("gather rc: %s\n", g_err); return 1; }
    float* pred = amalloc(m * Co * R);
    for (int i = 0; i < m; ++i) {
      const int* r = table + 4 * (g0 + i);
      for (int c = 0; c < C; ++c) for (int z = 0; z < rd; ++z) for (int y = 0; y < rh; ++y) for (int x = 0; x < rw; ++x) {
        float w = pad[((size_t)(r[0] * C + c) * P[0] + r[1] + z) * P[1] * P[2] + (size_t)(r[2] + y) * P[2] + r[3] + x];
        float g = win[(((size_t)(i * C + c) * rd + z) * rh + y) * rw + x];
        if (memcmp(&w, &g, 4)) ++bad;
      }
      for (int c = 0; c < Co; ++c) for (size_t e = 0; e < R; ++e) pred[((size_t)i * Co + c) * R + e] = win[((size_t)i * C + c % C) * R + e] * (c % 2 ? -0.25f : 0.5f) + 0.25f * c;
      for (int c = 0; c < Co; ++c) for (int z = 0; z < rd; ++z) for (int y = 0; y < rh; ++y) for (int x = 0; x < rw; ++x) {
        size_t e = ((size_t)z * rh + y) * rw + x;
        volatile float t = imap[e] * pred[((size_t)i * Co + c) * R + e];
        racc[((size_t)(r[0] * Co + c) * P[0] + r[1] + z) * P[1] * P[2] + (size_t)(r[2] + y) * P[2] + r[3] + x] += t;
        if (c == 0) rcnt[((size_t)r[0] * P[0] + r[1] + z) * P[1] * P[2] + (size_t)(r[2] + y) * P[2] + r[3] + x] += imap[e];
      }
    }
    if (gs_sw_accumulate(acc, B, Co, P[0], P[1], P[2], table + 4 * g0, table + 4 * g0, m, roi, imap, pred, nullptr)) { printf("acc rc: %s\n", g_err); return 1; }
    free(win); free(pred);
  }
  if (memcmp(acc, racc.data(), racc.size() * 4)) { printf("  accumulator differs\n"); ++bad; }
  float* res = amalloc(B * Co * V0); for (size_t i = 0; i < B * Co * V0; ++i) res[i] = NAN;
  if (gs_sw_finalize(acc, B, Co, D, H, W, table, n, roi, pb, imap, res, nullptr)) { printf("fin rc: %s\n", g_err); return 1; }
  for (int b = 0; b < B; ++b) for (int c = 0; c < Co; ++c) for (int z = 0; z < D; ++z) for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
    size_t q = ((size_t)z + pb[0]) * P[1] * P[2] + (size_t)(y + pb[1]) * P[2] + x + pb[2];
    want[((size_t)(b * Co + c) * D + z) * H * W + (size_t)y * W + x] = racc[(size_t)(b * Co + c) * VP + q] / rcnt[(size_t)b * VP + q];
  }
  if (memcmp(res, want.data(), want.size() * 4)) { printf("  result differs\n"); ++bad; }
  printf("B%d C%d->%d %dx%dx%d roi %dx%dx%d ov %.2f sw %d: n=%d %s\n", B, C, Co, D, H, W, rd, rh, rw, ov, sw, n, bad ? "FAIL" : "ok");
  free(in - misalign); free(imap); free(acc); free(res); free(table);
  return bad;
}
int main() {
  int bad = 0;
  bad += run_case(1, 1, 2, 20, 24, 28, 8, 16, 16, 0.25, 1, 0);
  bad += run_case(2, 2, 4, 17, 19, 23, 8, 8, 8, 0.5, 3, 0);
  bad += run_case(1, 1, 2, 12, 12, 12, 16, 8, 8, 0.25, 2, 0);
  bad += run_case(2, 3, 6, 1, 40, 56, 1, 16, 32, 0.25, 4, 0);
  bad += run_case(1, 1, 2, 16, 16, 16, 16, 16, 16, 0.25, 1, 0);
  bad += run_case(1, 1, 2, 30, 33, 35, 16, 16, 16, 0.0, 5, 0);
  bad += run_case(1, 2, 4, 9, 13, 11, 4, 7, 5, 0.4, 3, 0);
  bad += run_case(2, 1, 2, 8, 16, 32, 8, 8, 16, 0.5, 4, 0);
  bad += run_case(1, 2, 4, 5, 24, 24, 1, 16, 16, 0.25, 2, 0);
  bad += run_case(1, 2, 2, 5, 9, 5, 8, 4, 8, 0.25, 2, 0);      // z and x shorter than the roi
  bad += run_case(2, 1, 1, 4, 6, 10, 4, 4, 8, 0.75, 5, 0);     // unaligned quads
  bad += run_case(2, 1, 1, 4, 6, 12, 4, 4, 8, 0.5, 7, 1);      // input base not 16-byte aligned
  bad += run_case(1, 1, 1, 3, 3, 3, 5, 6, 7, 0.25, 1, 0);      // all axes shorter
  printf(bad ? "FAILED\n" : "ALL OK\n");
  return bad != 0;
}
