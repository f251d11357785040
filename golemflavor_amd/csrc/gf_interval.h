// Internal interface of gf_interval.hip (the column intervals of include/golemflavor_hip.h) for the entry points that own the rows
// they hand over: gf_column_intervals* and gf_sort_columns_device in gf_interval.hip itself, gf_sampler_intervals and
// gf_sampler_element_intervals in gf_postprocess.hip, gf_nested_intervals in gf_nested_post.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/golemflavor_hip.h"

// The two key buffers of a batch of chains stay under this many bytes (one chain at least); the chains of a call are processed batch
// after batch.  GF_INTERVAL_SCRATCH_BYTES in the environment overrides it (the batching changes, no result does).
#define GF_INTERVAL_SCRATCH_DEFAULT ((size_t)2 << 30)

// the public argument rules (spec may be NULL: sort only): GF_OK, GF_ERR_INVALID_ARG or GF_ERR_UNSUPPORTED
int gf_interval_check_args(int nchains, int64_t nrows, int width, const gf_interval_spec* spec);
// d_rows: chain ch's rows [nrows][width] start at d_rows + ch * chain_stride (doubles); everything on `st` (current device);
// spec != NULL: the intervals into *out (every pointer may be NULL); d_sorted != NULL: the sorted columns [nchains][width][nrows];
// synchronous
int gf_interval_run(hipStream_t st, const double* d_rows, int64_t chain_stride, int nchains, int64_t nrows, int width, const gf_interval_spec* spec,
                    const gf_interval_out* out, double* d_sorted);
