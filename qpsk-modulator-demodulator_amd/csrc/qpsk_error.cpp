// qpsk_error.cpp -- the error channel of the C ABI: one message per calling
// thread.  Host-only, so that the device-free entry points (the state-blob
// check, the design math) link without the HIP runtime.
#include <string>

#include "qpsk_demod.h"
#include "qpsk_internal.h"

namespace {
thread_local std::string g_last_error;
}  // namespace

int qpsk::fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

extern "C" const char *qpsk_last_error(void) { return g_last_error.c_str(); }
