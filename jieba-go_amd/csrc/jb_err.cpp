// jb_err.cpp — the calling thread's last error.  Host only, no HIP.
#include "jb_err.h"

#include <stdarg.h>
#include <stdio.h>

#include "../../include/jiebahip.h"

thread_local std::string g_err = "";

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char* jb_last_error(void) { return g_err.c_str(); }
