// hostcheck.h -- the host-side checks an entry point makes before it launches anything: sizes, pointers, alignment, scratch
// capacity.  Plain host C++ (no HIP): every function sets the thread's error text (dm4d_last_error) and returns true when it
// refuses, so an entry point reads `if (bad_count(fn, "N", N)) return DM4D_ERR_INVALID;`.  The texts are part of the ABI's
// behaviour (tests/test_host_refusals_cpu.py, tests/test_mesh_clean_cpu.py pin them).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dm4d {

void set_error(const char *fmt, ...);

// true (with the error set) for a size outside [0, most]
static inline bool bad_count(const char *fn, const char *what, int64_t n, int64_t most = INT32_MAX)
{
    if (n >= 0 && n <= most) return false;
    set_error("%s: %s = %lld is outside [0, %lld]", fn, what, (long long)n, (long long)most);
    return true;
}

// workgroups of `threads` that cover n items
static inline unsigned blocks(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// `bytes` is a power of two
static inline bool misaligned(const void *p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) != 0; }

// true (with the error set) when the caller's scratch is smaller than the call needs: the entry point returns DM4D_ERR_CAPACITY
static inline bool short_scratch(const char *fn, int64_t have, int64_t need)
{
    if (have >= need) return false;
    set_error("%s: scratch of %lld bytes, %lld needed", fn, (long long)have, (long long)need);
    return true;
}

// One pointer argument of an entry point.  bad_args refuses, by name and in table order, the first that is null while the call
// would read or write behind it, or that is not aligned.
struct Arg {
    const char *name;
    const void *p;
    unsigned align;
    int64_t n;          // elements behind the pointer: a null pointer is refused only when n > 0
};

template <size_t N>
static bool bad_args(const char *fn, const Arg (&args)[N])
{
    for (const Arg &a : args) {
        if (!a.p) {
            if (a.n > 0) { set_error("%s: %s is null", fn, a.name); return true; }
            continue;
        }
        if (misaligned(a.p, a.align)) { set_error("%s: %s is not %u-byte aligned", fn, a.name, a.align); return true; }
    }
    return false;
}

}  // namespace dm4d

// the anonymous refusal of the entry points that do not use the table; `fn` is the entry point's name
#define DM4D_REFUSE_NULL(cond)                          \
    if (cond) {                                         \
        dm4d::set_error("%s: null argument", fn);       \
        return DM4D_ERR_INVALID;                        \
    }
