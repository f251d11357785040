// gf_pool.h -- what gf_model.hip and gf_capi.hip need of the per-device pools (gf_pool.hip): the device's identity, pooled streams and
// constant blocks, and the unitarity workspace of a stream.  Internal to the library and not exported from it; everybody else goes
// through the gf_internal_* functions of gf_internal.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>

#include "gf_consts.h"

#define GF_LOCAL __attribute__((visibility("hidden")))

// a model's constant block: d_ptab [GF_MAX_DIM][4] | GfBsm | GfCommon, each 256-byte aligned
constexpr size_t CONST_PTAB_BYTES = sizeof(double) * GF_MAX_DIM * 4;
constexpr size_t CONST_BSM_OFFSET = (CONST_PTAB_BYTES + 255) / 256 * 256;
constexpr size_t CONST_COMMON_OFFSET = (CONST_BSM_OFFSET + sizeof(GfBsm) + 255) / 256 * 256;
constexpr size_t CONST_BLOCK_BYTES = CONST_COMMON_OFFSET + sizeof(GfCommon);

// GF_OK and *cus when `device` is a gfx950
GF_LOCAL int pool_device(int device, int* cus);
// an idle stream / constant block (CONST_BLOCK_BYTES) of the device's pool, or a new one
GF_LOCAL hipError_t pool_stream(int device, hipStream_t* stream);
GF_LOCAL hipError_t pool_block(int device, void** block);
// back to the pool (either may be NULL); the stream must be idle (the caller synchronised it)
GF_LOCAL void pool_release(int device, hipStream_t stream, void* block);

// The unitarity workspace of a stream, sized for one status batch and locked until the lease goes out of scope: what gf_launch_bsm
// takes besides the caller's arrays.
struct GfUniLease {
    std::unique_lock<std::mutex> lock;
    GfArbQueue* d_uq = nullptr;
    int64_t uq_items = 0;            // items of the arbitration queue a piece of the batch may use
    GfUniQueue* d_wq = nullptr;      // NULL for a batch whose tier 2 runs inside the evaluation kernel
    int64_t wq_cap = 0;
    double* d_t2sn = nullptr;
    unsigned int* h_seen = nullptr;
};
// Reports (and consumes) a stale overflow of an earlier asynchronous launch on `stream`, then locks the workspace and sizes it for `n`
// rows; hold the lease until the last launch that uses it is enqueued.
GF_LOCAL int pool_lease_workspace(int device, hipStream_t stream, int layout, int64_t n, GfUniLease* lease);
// Did an arbitration launch on this stream report a full queue?  Call after a stream synchronise.  The report is consumed.
GF_LOCAL int check_queue_overflow(int device, hipStream_t stream);
