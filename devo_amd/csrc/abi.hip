// What every part of libdevo_hip.so shares with its caller: the ABI version, the per-thread error text behind devo_last_error
// (written by set_error, common.h) and the stream-capture query.
#include "common.h"
#include <stdarg.h>

namespace devo {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

}  // namespace devo

using namespace devo;

extern "C" {

int devo_abi_version(void) { return DEVO_ABI_VERSION; }
const char* devo_last_error(void) { return g_err; }
int devo_stream_capturing(devo_stream_t stream) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess) { (void)hipGetLastError(); return -1; }
  return st == hipStreamCaptureStatusNone ? 0 : 1;
}

}  // extern "C"
