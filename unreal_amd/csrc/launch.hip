// The launch label (common.h: UNREAL_LAUNCHED): which template instantiation a launcher chose for its shape, stride and
// alignment, so that a test can assert that a shape lands on the variant it was chosen for.
#include <string.h>

#include "common.h"

thread_local const char* unreal_launch_label = "";

extern "C" int unreal_last_launch(char* buf, int len, void* stream) {
  (void)stream;
  if (!buf || len <= 0) return UNREAL_EINVAL;
  const char* s = unreal_launch_label ? unreal_launch_label : "";
  const size_t n = strnlen(s, (size_t)len - 1);
  memcpy(buf, s, n);
  buf[n] = '\0';
  return UNREAL_OK;
}
