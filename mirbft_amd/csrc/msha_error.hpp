// The exception an entry point's body throws: a return code of mirsha.h and the text that
// becomes the context's error. Host-only and HIP-free, so the host planning (host_plan.hpp)
// can throw it; host_call.hpp maps it to the return code (guard()).
#pragma once
#include <stdexcept>
#include <string>

namespace msha {

struct MshaError : std::runtime_error {
  int code;
  MshaError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

}  // namespace msha
