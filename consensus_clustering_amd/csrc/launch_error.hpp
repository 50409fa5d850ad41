// launch_error: the HIP error that the launches of an entry point left behind, as libccmi reports
// it.  For the .hip translation units (ccmi_internal.h is also compiled as plain C++).
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "ccmi_internal.h"

namespace {

int launch_error(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    cc::set_error(std::string(what) + ": " + hipGetErrorString(e));
    return CC_ERR_HIP;
  }
  return CC_OK;
}

}  // namespace
