// The native code's one exception type and its codes.  No HIP include, so the host-only headers
// (paged_view_host.h) and the stand-alone programs that compile them can throw it.
#pragma once
#include <stdexcept>
#include <string>

namespace amdx {

struct StoreError : std::runtime_error {
  int code;
  StoreError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
// error codes mirrored in Python (alluxio_amd/ops/native.py)
enum ErrCode {
  kErrNotFound = 1,
  kErrAlreadyExists = 2,
  kErrOutOfSpace = 3,
  kErrInvalidState = 4,
  kErrHip = 5,
  kErrInvalidArgument = 6,
  kErrIo = 7,
  kErrTimeout = 8,
};

}  // namespace amdx
