// Host-side helpers of the recurrent translation units (lt_memory_tile.h's and lt_seq_tile.h's entry points, lt_policy.hip): the named
// refusal of an argument before anything is launched, and the status of the launches issued.  Internal: an unnamed namespace.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "lt_env.h"
#include "lt_internal.h"

namespace {

// LT_EINVAL with "<fn>: invalid argument: <who><field> must be <what>"
int refuse(const char* fn, const char* who, const char* field, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: invalid argument: %s%s must be %s", fn, who, field, what);
  lt_set_error(msg);
  return LT_EINVAL;
}

struct ptr_check { const char* name; const void* p; int align; };

int check_ptr(const char* fn, const char* who, const ptr_check& e) {
  if (!e.p || (uintptr_t)e.p % e.align != 0) return refuse(fn, who, e.name, e.align == 16 ? "non-null and 16-byte aligned" : "non-null and 4-byte aligned");
  return LT_OK;
}

template <int n> int check_ptrs(const char* fn, const char* who, const ptr_check (&ptrs)[n]) {
  for (const auto& e : ptrs)
    if (const int rc = check_ptr(fn, who, e)) return rc;
  return LT_OK;
}

int launch_status() {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { lt_set_error(hipGetErrorString(e)); return LT_EHIP; }
  return LT_OK;
}

}  // namespace
