// Library identity and thread-local error reporting for the C-ABI.
#include <string.h>

#include "common.h"

namespace jabd {
static thread_local char g_err[512] = {0};

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

thread_local LaunchLog g_launch_log = {};
}  // namespace jabd

extern "C" int jabd_launch_log_reset(void) {
  jabd::g_launch_log.count = 0;
  return JABD_OK;
}

extern "C" int64_t jabd_launch_log_count(void) { return jabd::g_launch_log.count; }

// i counts launches since the reset; only the last kLaunchLogCap are kept
static bool launch_log_kept(int32_t i) {
  const int64_t n = jabd::g_launch_log.count;
  return i >= 0 && i < n && i >= n - jabd::kLaunchLogCap;
}

extern "C" const char* jabd_launch_log_name(int32_t i) {
  return launch_log_kept(i) ? jabd::g_launch_log.name[i & (jabd::kLaunchLogCap - 1)] : nullptr;
}

extern "C" int jabd_launch_log_tag(int32_t i) {
  return launch_log_kept(i) ? jabd::g_launch_log.tag[i & (jabd::kLaunchLogCap - 1)] : 0;
}

extern "C" const char* jabd_version(void) { return "jabd-mi355x 0.1.0 (gfx950)"; }

extern "C" int jabd_last_error(char* buf, size_t len) {
  if (!buf || len == 0) return JABD_EINVAL;
  strncpy(buf, jabd::g_err, len - 1);
  buf[len - 1] = 0;
  return JABD_OK;
}

// Sizes of the argument structs, so bindings can check their mirrors.
extern "C" int64_t jabd_abi_struct_size(int32_t which) {
  switch (which) {
    case 0: return (int64_t)sizeof(jabd_conv_args);
    case 1: return (int64_t)sizeof(jabd_dw_args);
    case 2: return (int64_t)sizeof(jabd_expdw_args);
    case 3: return (int64_t)sizeof(jabd_window_copy);
    default: return -1;
  }
}
