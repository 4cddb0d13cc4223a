// kmp_status.hip -- the library's status plumbing: the thread-local error text and launch name every C
// entry point leaves behind (kmp_common.h: set_error / fail / check_launch) and the entry points that read
// them back or need no kernel.  kmp_device_ok probes a kernel and lives with one (kmp_primitives.hip).
#include "kmp_common.h"

namespace kmp {

static thread_local std::string g_last_error;
static thread_local const char* g_last_launch = "";

void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int status, const std::string& msg) {
  g_last_error = msg;
  return status;
}
int check_launch(const char* what) {
  g_last_launch = what;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KMP_ERR_LAUNCH, std::string(what) + ": " + hipGetErrorString(e));
  return KMP_OK;
}

}  // namespace kmp

using namespace kmp;

extern "C" {

#ifdef KMP_DEBUG
const char* kmp_version(void) { return "kompressor_hip 0.2.0 (gfx950, debug: device bounds checks)"; }
#else
const char* kmp_version(void) { return "kompressor_hip 0.2.0 (gfx950)"; }
#endif
const char* kmp_last_error(void) { return g_last_error.c_str(); }
const char* kmp_last_launch(void) { return g_last_launch; }

int kmp_host_device_pointer(void* host, void** device) {
  KMP_REQUIRE(host && device, "null pointer");
  hipError_t e = hipHostGetDevicePointer(device, host, 0);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(KMP_ERR_UNSUPPORTED, std::string("not device-mapped host memory: ") + hipGetErrorString(e));
  }
  return KMP_OK;
}

}  // extern "C"
