// error.cpp — the error channel of libmtx (mtx.h mtx_last_error) and the ABI
// version. No HIP: links into a plain host program (tests/host).
#include <stdarg.h>
#include <stdio.h>

#include "mtx.h"

static thread_local char g_err[1024] = "";

void mtx_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" {

int mtx_abi_version(void) { return MTX_ABI_VERSION; }

const char *mtx_last_error(void) { return g_err; }

}  // extern "C"
