// Library lifecycle + error plumbing for libganslate_hip.so (see include/ganslate_hip.h).
#include "internal.hpp"
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>

namespace {
thread_local char g_err[512] = "";   // per host thread: autograd runs backward launches on its own threads, and a caller
                                      // reads the message right after the failing call on the thread that made it
void* g_zero = nullptr;      // 256-byte zero page: source of masked LDS-DMA lanes
void* g_dump = nullptr;      // 256 writable bytes nobody reads
// Loss reductions: 1024 partials + 1 arrival counter per workspace. Launches on one stream are ordered and share a
// workspace; launches on different streams may overlap (the discriminator pass runs beside the generators' backward),
// so every stream that ever launched a reduction owns one of GS_WS_SLOTS workspaces.
constexpr int GS_WS_SLOTS = 256;     // torch hands out streams from pools of 32 per priority: far below this
constexpr int GS_WS_FLOATS = 1040;
float* g_reduce_ws = nullptr;
void* g_ws_stream[GS_WS_SLOTS] = {};
int g_ws_used = 0;
std::mutex g_ws_mutex;
}  // namespace

void gs_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
const void* gs_zero_page() { return g_zero; }
void* gs_dump_page() { return g_dump; }
float* gs_reduce_workspace(void* stream) {
  if (!g_reduce_ws) return nullptr;
  std::lock_guard<std::mutex> lock(g_ws_mutex);
  for (int i = 0; i < g_ws_used; ++i)
    if (g_ws_stream[i] == stream) return g_reduce_ws + (size_t)i * GS_WS_FLOATS;
  if (g_ws_used < GS_WS_SLOTS) {
    g_ws_stream[g_ws_used] = stream;
    return g_reduce_ws + (size_t)(g_ws_used++) * GS_WS_FLOATS;
  }
  // more launching streams than workspaces: two live streams would share partial sums, so refuse instead of aliasing
  gs_set_error("loss reductions were launched from more than %d streams of this process; raise GS_WS_SLOTS (api.hip)",
               GS_WS_SLOTS);
  return nullptr;
}

namespace {
struct OptDef { const char* name; int value; };
OptDef g_opts[GS_OPT_COUNT] = {       // one entry per row of GS_OPTIONS (common.hpp), in the enum's order by construction
#define GS_OPT_DEF(id, name, def) {name, def},
    GS_OPTIONS(GS_OPT_DEF)
#undef GS_OPT_DEF
};
}  // namespace
int gs_opt(int id) { return g_opts[id].value; }

extern "C" int gs_set_option(const char* name, int value) {
  for (int i = 0; i < GS_OPT_COUNT; ++i)
    if (name && strcmp(name, g_opts[i].name) == 0) { g_opts[i].value = value; return 0; }
  gs_set_error("gs_set_option: unknown option '%s'", name ? name : "(null)");
  return 2;
}
extern "C" int gs_get_option(const char* name, int* value) {
  for (int i = 0; i < GS_OPT_COUNT; ++i)
    if (name && value && strcmp(name, g_opts[i].name) == 0) { *value = g_opts[i].value; return 0; }
  gs_set_error("gs_get_option: unknown option '%s'", name ? name : "(null)");
  return 2;
}

extern "C" const char* gs_last_error(void) { return g_err; }

extern "C" int gs_init(int device) {
  GS_CHECK_HIP(hipSetDevice(device));
  if (!g_zero) {
    GS_CHECK_HIP(hipMalloc(&g_zero, 256));
    GS_CHECK_HIP(hipMemset(g_zero, 0, 256));
  }
  if (!g_dump) GS_CHECK_HIP(hipMalloc(&g_dump, 256));
  if (!g_reduce_ws) {
    GS_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&g_reduce_ws), GS_WS_SLOTS * GS_WS_FLOATS * sizeof(float)));
    GS_CHECK_HIP(hipMemset(g_reduce_ws, 0, GS_WS_SLOTS * GS_WS_FLOATS * sizeof(float)));
  }
  hipDeviceProp_t prop;
  GS_CHECK_HIP(hipGetDeviceProperties(&prop, device));
  GS_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0,
             "gs_init: device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
  return 0;
}

extern "C" void gs_shutdown(void) {
  if (g_zero) { (void)hipFree(g_zero); g_zero = nullptr; }
  if (g_dump) { (void)hipFree(g_dump); g_dump = nullptr; }
  if (g_reduce_ws) { (void)hipFree(g_reduce_ws); g_reduce_ws = nullptr; g_ws_used = 0; }
}
