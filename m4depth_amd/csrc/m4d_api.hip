// Library introspection entry points (no GPU work) and the table of environment switches.
#include <hip/hip_runtime.h>
#include "../../include/m4depth_hip.h"
#include "m4d_switches.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>

extern "C" int m4d_abi_version(void) { return M4D_ABI_VERSION; }

static std::atomic<long long> g_launches{0};
extern "C" __attribute__((visibility("hidden"))) void m4d_count_launch(void) { g_launches.fetch_add(1, std::memory_order_relaxed); }
extern "C" long long m4d_launch_count(void) { return g_launches.load(std::memory_order_relaxed); }

#define M4D_STR2(x) #x
#define M4D_STR(x) M4D_STR2(x)
#if defined(M4D_EXPERIMENTS) && M4D_EXPERIMENTS
#define M4D_FLAVOUR " +experiments"
#else
#define M4D_FLAVOUR ""
#endif
extern "C" const char* m4d_build_info(void) {
  return "libm4depth_hip gfx950 (CDNA4) -ffp-contract=off abi=" M4D_STR(M4D_ABI_VERSION) M4D_FLAVOUR " built " __DATE__ " " __TIME__;
}

// The only place the library reads the environment (m4d_switches.h).
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
const M4dSwitches& m4d_switches() {
  static const M4dSwitches table = [] {
    M4dSwitches t;
    t.sncv_variant = env_int("M4D_SNCV_VARIANT", 1);
    t.sncv_ys = env_int("M4D_SNCV_YS", 0);
    t.sncv_small_px = env_int("M4D_SNCV_SMALL_PX", 6000);
    t.wino_variant = env_int("M4D_WINO_VARIANT", 4);
    t.wino4_min_wg = env_int("M4D_WINO4_MIN_WG", 100);
    const int kb = env_int("M4D_DSCV_BWD_WINDOW_KB", 48);
    t.dscv_bwd_window_kb = kb < 0 ? 0 : (kb > 64 ? 64 : kb);
    return t;
  }();
  return table;
}

extern "C" const char* m4d_switches_info(void) {
  struct Text { char s[192]; };
  static const Text text = [] {
    const M4dSwitches& t = m4d_switches();
    Text x;
    snprintf(x.s, sizeof(x.s), "sncv_variant=%d sncv_ys=%d sncv_small_px=%d wino_variant=%d wino4_min_wg=%d dscv_bwd_window_kb=%d",
             t.sncv_variant, t.sncv_ys, t.sncv_small_px, t.wino_variant, t.wino4_min_wg, t.dscv_bwd_window_kb);
    return x;
  }();
  return text.s;
}
