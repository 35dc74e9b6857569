// ss_chart_dev.h: the chart-column rule, for every kernel that reduces dB values to the columns of the spectrum chart (ss_fft.hip,
// ss_util.hip, ss_spectrogram.hip, ss_bank_spectrum_track.hip).  DESIGN.md, "Chart columns".
//
// A column owns the bins whose chart_x falls into it (the map: ssh::column_starts / ssh::column_tables, ss_host.h) and shows the
// maximum over them of clamp(dB + gain, -100, 0) (tui.rs:49-51).  The gain is a fixed one or the reference's per-file rule
// FFT_TARGET_LUFS - integrated = -13 - (float)integrated, in f32 (tui.rs:1234).  Gain and clamp are monotone, so they commute
// with the maximum: the kernels that fold plain dB values into accumulators apply them ONCE per column, behind the fold —
// max(clamp(v + gain)) == clamp(max(v) + gain) to the bit.  An accumulator starts at -inf where the column owns a bin and at NaN
// where it owns none (col_init), and is folded with a float maximum that ignores a NaN operand: a NaN accumulator at the flush
// means "no bin".  The two clamps differ in what a NaN SUM (inf - inf) reads, see chart_cell and chart_cell_keep_nan.
#pragma once
#include "ss_kernels.h"

namespace ssk {
// the reference's gain for a file of this integrated loudness (the host forms a session's with it too)
__host__ __device__ __forceinline__ float chart_reference_gain(double integrated) { return -13.0f - (float)integrated; }
// the gain of a launch: the reference's from integrated[index], or gain_db where integrated is null
__device__ __forceinline__ float chart_gain(const double *integrated, size_t index, float gain_db) { return integrated ? chart_reference_gain(integrated[index]) : gain_db; }
__device__ __forceinline__ float chart_gain(const ChartFold &f, uint32_t stream) { return chart_gain(f.integrated, (size_t)stream * f.integrated_stride, f.gain_db); }
// the chart's clamp, fminf / fmaxf (minNum / maxNum): a NaN operand reads -100
__device__ __forceinline__ float chart_clamp(float x) { return fminf(fmaxf(x, -100.0f), 0.0f); }
// a column's folded maximum k as its cell: a NaN k (the column owns no bin) stays; a NaN sum reads -100, as in the two-pass kernel
__device__ __forceinline__ float chart_cell(float k, float gain) { return k != k ? k : chart_clamp(k + gain); }
// the spectrogram's form, compare and select like numpy's clip: a NaN — no value, or inf - inf — stays NaN
__device__ __forceinline__ float chart_cell_keep_nan(float k, float gain)
{
    float x = k + gain;
    x = x < -100.0f ? -100.0f : x;
    return x > 0.0f ? 0.0f : x;
}
// the accumulators' fold: an LDS float maximum (ds_max_f32), which ignores a NaN operand like IEEE maxNum
typedef __attribute__((address_space(3))) float lds_f32;
__device__ __forceinline__ void lds_fmax(lds_f32 *p, float v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
}  // namespace ssk
