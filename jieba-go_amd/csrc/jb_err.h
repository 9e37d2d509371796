// jb_err.h — the calling thread's last error (jb_last_error).  Library-internal.
#pragma once
#include <string>

#pragma GCC visibility push(hidden)

// Thread-local: a worker thread hands its message to the caller's thread by copying g_err.
extern thread_local std::string g_err;

// Sets the thread's message and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#pragma GCC visibility pop

#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t _e = (x);                                                                   \
        if (_e != hipSuccess) return fail(JB_EDEVICE, "%s: %s", #x, hipGetErrorString(_e));   \
    } while (0)
