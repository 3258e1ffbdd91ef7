// lab_host.hpp -- host-side helpers the Lab family's translation units share (lab.hip, slide_lab.hip, lab_view.hip).
#pragma once
#include "lab_device.hpp"
#include "sl_host.hpp"

namespace sl {

// n >= 0 tiles of h x w: the shape checks every entry point with a shard shares
inline bool slab_shape_ok(int n, int h, int w) {
    if (n < 0 || h <= 0 || w <= 0) return false;
    const long P = (long)h * w;
    return P <= (1L << 30) && (long)n * P <= (1L << 40);
}

// ---- lab.hip, for the entry points that put another map behind its statistics (lab_view.hip) ----------------------------------------
// the checks of every per-tile entry point with a workspace
int lab_check(const void* rgb, const void* out, int n, int h, int w, const void* ws, size_t ws_bytes);
// the per-tile tables in a workspace lab_check has accepted
LabTileTabs* lab_tabs_of(void* ws, int n);
// sl_reinhard_transform up to its map: the two statistics sweeps, k_lab_stats when stats_out is given, k_lab_tables<0>
int lab_reinhard_tables(const uint8_t* rgb, int n, long P, const double* target_means, const double* target_stds, double thr,
                        double* stats_out, void* ws, hipStream_t s);
// sl_luminosity_standardize up to its map: the L8 histogram sweep, k_lab_tables<1>
int lab_luminosity_tables(const uint8_t* rgb, int n, long P, double percentile, void* ws, hipStream_t s);

}  // namespace sl
