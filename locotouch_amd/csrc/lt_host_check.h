// Host-side checks of every translation unit that answers with an LT_* status: the refusal of an argument before anything is launched
// (three forms, by how the unit words its message) and the status of the launches issued.  Internal: an unnamed namespace.  The
// launchers that hand back a raw hipError_t (lt_internal.h) do not come through here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "lt_env.h"
#include "lt_internal.h"

namespace {

// LT_EINVAL with `msg` as it stands
int einval(const char* msg) {
  lt_set_error(msg);  // (copies)
  return LT_EINVAL;
}

// LT_EINVAL with "<fn>: <what>"
int refuse(const char* fn, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", fn, what);
  return einval(msg);
}

// LT_EINVAL with "<fn>: invalid argument: <who><field> must be <what>"
int refuse(const char* fn, const char* who, const char* field, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: invalid argument: %s%s must be %s", fn, who, field, what);
  return einval(msg);
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

// LT_EHIP if a launch since the last look failed, with the HIP error string - behind "<fn>: " where the unit names its entry point
int launch_status(const char* fn = nullptr) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return LT_OK;
  char msg[256];
  if (fn) snprintf(msg, sizeof msg, "%s: %s", fn, hipGetErrorString(e));
  lt_set_error(fn ? msg : hipGetErrorString(e));
  return LT_EHIP;
}

}  // namespace
