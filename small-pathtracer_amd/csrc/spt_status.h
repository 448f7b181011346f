// spt_status.h — the error path of everything behind the C ABI, stated once. Internal, and HIP-free
// to include: the files the stand-alone programs of tests/probe/ build with plain host clang include
// it too. SPT_HIP names HIP only where it is used.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/spt.h"

void spt_set_last_error(const std::string& msg);  // spt_dispatch.cpp: spt_last_error()'s text
int spt_shard_row_count(const spt_params* p);     // spt_host.cpp: the rows of p's shard
inline int tile_rows_of(const spt_params* p) { return p->tile_rows > 0 ? p->tile_rows : 8; }

namespace spt {

spt_status fail(spt_status s, const std::string& msg);  // spt_dispatch.cpp: sets the text, returns s

// ---- spt_context.cpp (stream: a hipStream_t, kind: a hipMemcpyKind)
// What every create call opens with: count the devices, check the ordinal, make it current.
// say_why: the "no HIP device" text carries the HIP error string (the encoder's).
spt_status open_device(int32_t device, bool say_why = false);
// Copy a plane to or from the host on `device` and wait for the stream.
spt_status copy_and_wait(int device, void* dst, const void* src, size_t bytes, int kind, void* stream);

}  // namespace spt

#define SPT_TRY(expr)                   \
  do {                                  \
    const spt_status st_ = (expr);      \
    if (st_ != SPT_OK) return st_;      \
  } while (0)

#define SPT_HIP(call)                                                                    \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess)                                                                \
      return spt::fail(e_ == hipErrorOutOfMemory ? SPT_ERR_OOM : SPT_ERR_HIP,            \
                       std::string(#call) + ": " + hipGetErrorString(e_));               \
  } while (0)
