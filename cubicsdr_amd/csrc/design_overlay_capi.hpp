// design_overlay_capi.hpp -- the C entry points of the overlay planners (design.hpp; include/csdr_hip.h, "Overlay bank", a - e), stated once and
// compiled into both libraries: the host-only design library (design_capi.cpp) and the GPU library (csdr_overlay.hip), where the host mirror and
// the Python binding find them next to csdr_overlay_compose.  Host code only; no device, no context, no csdr_last_error.
#pragma once
#include "design.hpp"

extern "C" {

int csdr_design_freq_scale(int64_t freq, int64_t bandwidth, int view_w, int view_h, double font_scale, csdr_freq_scale *out, csdr_freq_tick *ticks, int cap) {
    return csdr::design::freq_scale(freq, bandwidth, view_w, view_h, font_scale, out, ticks, cap);
}
int csdr_design_db_grid(float floor_value, float ceil_value, csdr_db_grid_range *ranges, int *n_ranges, double *p, int cap) {
    return csdr::design::db_grid(floor_value, ceil_value, ranges, n_ranges, p, cap);
}
int csdr_design_db_labels(float floor_value, float ceil_value, int fft_size, double db_offset, char *ceil_label, char *floor_label, int cap) {
    return csdr::design::db_labels(floor_value, ceil_value, fft_size, db_offset, ceil_label, floor_label, cap);
}
int csdr_design_demod_marker(int64_t demod_freq, int bandwidth, int sideband, int64_t center_freq, int64_t srate, int flags, int view_w, int view_h,
                             const uint8_t *rgb, csdr_demod_marker *out, csdr_overlay_prim *prims, int *n_prims) {
    return csdr::design::demod_marker(demod_freq, bandwidth, sideband, center_freq, srate, flags, view_w, view_h, rgb, out, prims, n_prims);
}
int csdr_design_text(const csdr_glyph *glyphs, int n_glyphs, int line_height, const char *str, int x, int y, int halign, int valign, const uint8_t *rgba, int mode,
                     csdr_overlay_prim *out, int cap, int *n_out) {
    return csdr::design::text_prims(glyphs, n_glyphs, line_height, str, x, y, halign, valign, rgba, mode, out, cap, n_out);
}

}  // extern "C"
