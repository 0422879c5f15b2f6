// sugar_reg_host_check.cpp -- the host-side argument checks of csrc/sugar_reg.hip under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a stand-alone program (no device is touched: every call below returns before a launch).
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Xarch_host -fsanitize=address,undefined \
//         dreammesh4d_amd/csrc/sugar_reg.hip tools/sugar_reg_host_check.cpp -o build/sugar_reg_host_check && build/sugar_reg_host_check
//
// Prints "ok: <n> calls" and exits 0 when every call returned what it should and neither sanitizer reported anything.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "dm4d.h"
#include "dm4d_sugar_reg.h"

static char g_error[512];
namespace dm4d {
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
}  // namespace dm4d

static int g_calls = 0, g_failed = 0;
static void expect(const char *what, long long got, long long want, const char *fn)
{
    ++g_calls;
    const bool named = want >= 0 || strstr(g_error, fn) != nullptr;
    if (got != want || !named) {
        ++g_failed;
        printf("FAILED %s: returned %lld, expected %lld (message: %s)\n", what, got, want, g_error);
    }
    g_error[0] = 0;
}

int main()
{
    void *P = reinterpret_cast<void *>(0x1000);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const int64_t big = (int64_t)1 << 40;
    expect("version", dm4d_sr_version(), DM4D_SR_ABI_VERSION, "");
    const int64_t sizes[][3] = {{-1, 16, 8}, {(int64_t)DM4D_SR_MAX_POINTS + 1, 16, 8}, {4, 0, 8}, {4, 33, 8}, {4, 16, -1},
                                {4, 16, (int64_t)DM4D_SR_MAX_SAMPLES + 1}, {INT64_MIN, 1, 1}, {1, 1, INT64_MAX}};
    for (const auto &s : sizes) {
        expect("scratch_bytes sizes", dm4d_sr_scratch_bytes(s[0], (int32_t)s[1], s[2]), DM4D_ERR_INVALID, "dm4d_sr_scratch_bytes");
        expect("forward sizes", dm4d_sr_forward(s[0], (int32_t)s[1], s[2], P, P, P, P, P, P, P, P, 1.5f, 1.0f, 0, P, big, P, P, P, P, P, nullptr),
               DM4D_ERR_INVALID, "dm4d_sr_forward");
        expect("backward sizes", dm4d_sr_backward(s[0], (int32_t)s[1], s[2], P, P, P, P, P, P, P, P, 1.5f, 1.0f, 0, P, P, P, P, P, P, big, P, P, P, P, nullptr),
               DM4D_ERR_INVALID, "dm4d_sr_backward");
    }
    const int64_t largest = dm4d_sr_scratch_bytes(DM4D_SR_MAX_POINTS, DM4D_SR_MAX_K, DM4D_SR_MAX_SAMPLES);
    expect("scratch_bytes at the limits is positive", largest > 0, 1, "");
    const int64_t need = dm4d_sr_scratch_bytes(400, 16, 3000);
    expect("scratch_bytes is a multiple of 256", need % 256, 0, "");
    const float scalars[][2] = {{nan, 1.0f}, {inf, 1.0f}, {-inf, 1.0f}, {1.5f, nan}, {1.5f, inf}};
    for (const auto &s : scalars) {
        expect("forward scalars", dm4d_sr_forward(4, 2, 8, P, P, P, P, P, P, P, P, s[0], s[1], 0, P, big, P, P, P, P, P, nullptr), DM4D_ERR_INVALID, "dm4d_sr_forward");
        expect("backward scalars", dm4d_sr_backward(4, 2, 8, P, P, P, P, P, P, P, P, s[0], s[1], 0, P, P, P, P, P, P, big, P, P, P, P, nullptr), DM4D_ERR_INVALID, "dm4d_sr_backward");
    }
    for (int flag : {-1, 2, INT32_MAX}) {
        expect("forward flag", dm4d_sr_forward(4, 2, 8, P, P, P, P, P, P, P, P, 1.5f, 1.0f, flag, P, big, P, P, P, P, P, nullptr), DM4D_ERR_INVALID, "dm4d_sr_forward");
        expect("backward flag", dm4d_sr_backward(4, 2, 8, P, P, P, P, P, P, P, P, 1.5f, 1.0f, flag, P, P, P, P, P, P, big, P, P, P, P, nullptr), DM4D_ERR_INVALID, "dm4d_sr_backward");
    }
    for (int null = 0; null < 13; ++null) {                   // each pointer of the forward in turn
        void *p[13];
        for (auto &v : p) v = P;
        p[null] = nullptr;
        const int normal = null == 11 ? 1 : 0;                // normal_term may be null without the normal loss
        expect("forward null", dm4d_sr_forward(4, 2, 8, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], 1.5f, 1.0f, normal, p[8], big, p[9], p[10], p[12], p[11], P, nullptr),
               DM4D_ERR_INVALID, "dm4d_sr_forward");
    }
    for (int null = 0; null < 14; ++null) {                   // each required pointer of the backward in turn
        void *p[14];
        for (auto &v : p) v = P;
        p[null] = nullptr;
        expect("backward null", dm4d_sr_backward(4, 2, 8, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], 1.5f, 1.0f, 1, p[8], p[9], p[10], p[11], p[12], p[13], big, P, P, P, P, nullptr),
               DM4D_ERR_INVALID, "dm4d_sr_backward");
    }
    expect("forward misaligned scratch", dm4d_sr_forward(4, 2, 8, P, P, P, P, P, P, P, P, 1.5f, 1.0f, 0, (char *)P + 4, big, P, P, P, P, P, nullptr), DM4D_ERR_INVALID, "dm4d_sr_forward");
    expect("forward small scratch", dm4d_sr_forward(400, 16, 3000, P, P, P, P, P, P, P, P, 1.5f, 1.0f, 0, P, need - 1, P, P, P, P, P, nullptr), DM4D_ERR_CAPACITY, "dm4d_sr_forward");
    expect("backward small scratch", dm4d_sr_backward(400, 16, 3000, P, P, P, P, P, P, P, P, 1.5f, 1.0f, 0, P, P, P, P, P, P, 0, P, P, P, P, nullptr), DM4D_ERR_CAPACITY, "dm4d_sr_backward");
    expect("backward negative scratch", dm4d_sr_backward(400, 16, 3000, P, P, P, P, P, P, P, P, 1.5f, 1.0f, 0, P, P, P, P, P, P, INT64_MIN, P, P, P, P, nullptr), DM4D_ERR_CAPACITY, "dm4d_sr_backward");
    expect("forward N = 0", dm4d_sr_forward(0, 16, 8, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1.5f, 1.0f, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), DM4D_OK, "");
    expect("backward S = 0", dm4d_sr_backward(4, 16, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1.5f, 1.0f, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr), DM4D_OK, "");
    if (g_failed) {
        printf("%d of %d calls failed\n", g_failed, g_calls);
        return 1;
    }
    printf("ok: %d calls\n", g_calls);
    return 0;
}
