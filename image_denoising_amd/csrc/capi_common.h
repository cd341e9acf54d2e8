// What the files of the extern "C" boundary (capi_*.cpp, profile.cpp) share (internal).  The
// boundary validates arguments and maps failures to dn_status + a thread-local message; no C++
// exception leaves it: every entry point's body runs inside guarded() or guarded_query().
#pragma once
#include <exception>
#include <string>

#include "exec_common.h"

namespace dn {

inline dn_status fail(int code, const std::string& msg) {
  set_error(msg);
  return code;
}

inline dn_status hip_status(hipError_t e, const char* what) {
  if (e == hipSuccess) return DN_OK;
  return fail(DN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// the exception barrier of a dn_status entry point: body's status, or DN_ERR_ARG with the
// exception's text
template <class Body>
dn_status guarded(Body&& body) {
  try {
    return body();
  } catch (const std::exception& ex) {
    return fail(DN_ERR_ARG, ex.what());
  } catch (...) {
    return fail(DN_ERR_ARG, "unknown C++ exception");
  }
}

// the same for a size or count query, which has no status to return: 0 on an exception
template <class Body>
auto guarded_query(Body&& body) -> decltype(body()) {
  try {
    return body();
  } catch (...) {
    return 0;
  }
}

}  // namespace dn
