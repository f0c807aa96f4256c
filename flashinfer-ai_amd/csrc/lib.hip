// Error channel, kernel-choice switches and device queries of libfi_mi355.so.  Host code only.
#include <errno.h>
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "common.h"

namespace fi {

static thread_local char g_err[1024] = "";

int set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return 1;
}
const char* last_error() { return g_err; }

// ---- the switch table: one entry per Option and in its order, named as its environment variable ----
static const char* const kOptionNames[OPT_COUNT] = {
    "FI_NUM_CUS",           "FI_DECODE_MFMA16",      "FI_GEMM_WS_MIN_TILES",       "FI_GEMM_DMA_TM",
    "FI_GEMM_BIG",          "FI_GEMM_BIG_MIN_TILES", "FI_GEMM_BIG_FOLD_MIN_TILES", "FI_GEMM_HW_SCALES",
    "FI_MM_FP4_KERNEL"};
constexpr int64_t kUnset = INT64_MIN;     // no int: an entry holds an int or this
static int64_t g_env[OPT_COUNT];          // what the environment gave, written at load only
static std::atomic<int64_t> g_option[OPT_COUNT];

// the one reader of the environment: at load, before any call into the library
static const bool g_options_loaded = [] {
  for (int i = 0; i < OPT_COUNT; ++i) {
    const char* e = getenv(kOptionNames[i]);
    g_env[i] = e ? (int64_t)atoi(e) : kUnset;
    g_option[i].store(g_env[i], std::memory_order_relaxed);
  }
  return true;
}();

std::optional<int> option(Option o) {
  const int64_t v = g_option[o].load(std::memory_order_relaxed);
  return v == kUnset ? std::nullopt : std::optional<int>((int)v);
}

}  // namespace fi

extern "C" FI_API const char* fi_last_error(void) { return fi::last_error(); }
extern "C" FI_API int fi_abi_version(void) { return FI_ABI_VERSION; }

extern "C" FI_API int fi_set_option(const char* name, const char* value) {
  FI_REQUIRE(name, "fi_set_option: null name");
  int o = 0;
  while (o < fi::OPT_COUNT && strcmp(name, fi::kOptionNames[o]) != 0) ++o;
  FI_REQUIRE(o < fi::OPT_COUNT, "fi_set_option: unknown option '%s'", name);
  int64_t v = fi::g_env[o];
  if (value) {
    char* end = nullptr;
    errno = 0;
    const long parsed = strtol(value, &end, 10);
    FI_REQUIRE(end != value && *end == '\0' && errno == 0 && parsed >= INT_MIN && parsed <= INT_MAX,
               "fi_set_option: %s='%s' is not an integer", name, value);
    v = parsed;
  }
  fi::g_option[o].store(v, std::memory_order_relaxed);
  return 0;
}

extern "C" FI_API int fi_num_compute_units(void) {
  if (const int v = fi::option(fi::OPT_NUM_CUS).value_or(0); v > 0) return v;
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
    return n;
  (void)hipGetLastError();
  return 256;  // MI355X
}
