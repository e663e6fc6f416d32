// The environment switches of the library: one table, read once.
//
// m4d_switches() reads the M4D_* variables below on its first call (thread-safe initialisation of a function-local
// static const) and never writes the table again: entry points stay callable from any host thread, and a variable set
// after the first call has no effect.  A switch is kept only while a test, a tool or bench.py sets it (INTEGRATION.md,
// "Switches of the library itself"); m4d_switches_info() reports the values a process runs with.  No other translation
// unit of the library reads the environment.
#pragma once

struct M4dSwitches {
  int sncv_variant;         // M4D_SNCV_VARIANT        1     0 = no specialised SNCV kernel (debugging)
  int sncv_ys;              // M4D_SNCV_YS             0     1 | 2 | 4 = window-row split of the 7x7 SNCV kernel, 0 = by size
  int sncv_small_px;        // M4D_SNCV_SMALL_PX       6000  maps up to this many pixels (batch included) take the small-map kernels
  int wino_variant;         // M4D_WINO_VARIANT        4     2 = Winograd kernel 2 at every grid size
  int wino4_min_wg;         // M4D_WINO4_MIN_WG        100   grids of at least this many workgroups take Winograd kernel 4
  int dscv_bwd_window_kb;   // M4D_DSCV_BWD_WINDOW_KB  48    LDS window of the DSCV backward, KB, clamped to 0..64; 0 = direct scatter
};

__attribute__((visibility("hidden"))) const M4dSwitches& m4d_switches();
