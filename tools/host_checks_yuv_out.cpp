// host_checks_yuv_out.cpp -- the host side of the planar YUV image output under AddressSanitizer / UBSan, as a stand-alone program:
// the coefficient builder (ncahip_rgb_yuv_coeffs) against include/ncahip.h's table, and every refusal of the entry points that take
// the new image formats.  Every call here ends at a host-side check: nothing is launched and no pointer is dereferenced, so the program
// needs no GPU.  Built by `make -C video-stylization-with-nca_amd host-asan` (host code instrumented, device code as always).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "ncahip.h"

static int failures = 0;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED line %d: %s   (last error: %s)\n", __LINE__, #cond, ncahip_last_error()); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static void* P(uintptr_t a) { return reinterpret_cast<void*>(a); }
static float* PF(uintptr_t a) { return reinterpret_cast<float*>(a); }
static bool said(const char* word) { return std::strstr(ncahip_last_error(), word) != nullptr; }

int main() {
    static const int32_t table[4][10] = {{16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681, 16},
                                         {19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329, 0},
                                         {11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639, 16},
                                         {13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005, 0}};
    for (int matrix = 0; matrix < 2; ++matrix)
        for (int range = 0; range < 2; ++range) {
            int32_t k[10];
            EXPECT(ncahip_rgb_yuv_coeffs(matrix, range, k) == 0);
            EXPECT(std::memcmp(k, table[2 * matrix + range], sizeof(k)) == 0);
        }
    int32_t k[10];
    EXPECT(ncahip_rgb_yuv_coeffs(2, 0, k) == NCAHIP_EINVAL && ncahip_rgb_yuv_coeffs(0, -1, k) == NCAHIP_EINVAL);
    EXPECT(ncahip_rgb_yuv_coeffs(0, 0, nullptr) == NCAHIP_EINVAL);
    EXPECT(ncahip_rgb_yuv_coeffs(1, 0, k) == 0);

    const uintptr_t st = 0x1000000, img = 0x3000000, gray = 0x2000000;
    const uint8_t* const src = static_cast<const uint8_t*>(P(0x10000));
    uint8_t* const dst = static_cast<uint8_t*>(P(0x800000));
    EXPECT(ncahip_clip_rgb_to_yuv420_u8(nullptr, 0, 2, 8, 10, k, dst, nullptr) == NCAHIP_EINVAL);
    EXPECT(ncahip_clip_rgb_to_yuv420_u8(src, 2, 2, 8, 10, k, dst, nullptr) == NCAHIP_EINVAL);
    EXPECT(ncahip_clip_rgb_to_yuv420_u8(src, 0, 0, 8, 10, k, dst, nullptr) == NCAHIP_EINVAL);
    EXPECT(ncahip_clip_rgb_to_yuv420_u8(src, 0, 2, 7, 10, k, dst, nullptr) == NCAHIP_ERANGE);
    EXPECT(ncahip_clip_rgb_to_yuv420_u8(src, 1, 2, 8, 16386, k, dst, nullptr) == NCAHIP_ERANGE);
    EXPECT(ncahip_clip_rgb_to_yuv420_u8(src, 1, 2, 8, 10, k, static_cast<uint8_t*>(P(0x10000 + 2 * 8 * 10 * 3 - 1)), nullptr) == NCAHIP_EINVAL && said("overlap"));

    for (int fmt = 0x100; fmt < 0x108; ++fmt) {
        const uintptr_t touching = st - 3 * 8 * 8 / 2 + 1;      // the planar image's last byte on the state's first
        EXPECT(ncahip_clip_emit(PF(st), P(touching), fmt, 1, 12, 3, 8, 8, nullptr) == NCAHIP_EINVAL && said("overlap"));
        EXPECT(ncahip_clip_emit(PF(st), P(img), fmt, 1, 12, 4, 8, 8, nullptr) == NCAHIP_EINVAL && said("3 channels"));
        EXPECT(ncahip_clip_emit(PF(st), P(img), fmt, 1, 12, 3, 7, 8, nullptr) == NCAHIP_ERANGE && said("even"));
        EXPECT(ncahip_clip_emit_inject(PF(st), P(touching), fmt, PF(gray), 1, 13, 3, 8, 8, nullptr) == NCAHIP_EINVAL && said("overlap"));
        EXPECT(ncahip_clip_emit_inject(PF(st), P(img), fmt, PF(gray), 1, 13, 3, 8, 9, nullptr) == NCAHIP_ERANGE);
        EXPECT(ncahip_clip_emit_unit(PF(st), P(touching), fmt, 1, 16, 8, 8, nullptr) == NCAHIP_EINVAL && said("overlap"));
        EXPECT(ncahip_clip_emit_unit(PF(st), P(img), fmt, 1, 16, 9, 9, nullptr) == NCAHIP_ERANGE);
        // the drivers: six planar images that end one byte before the state pass the overlap check and stop at the epoch check
        const uintptr_t before = st - 6 * 3 * 8 * 8 / 2;
        EXPECT(ncahip_dynca_clip_f32(PF(st), PF(gray), P(before), fmt, 3, 2, 4, nullptr, PF(0x4000000), PF(0x4100000), PF(0x4200000), PF(0x4300000), 1, 12, 3,
                                     8, 8, 96, 1, 0, 0.5f, 0, 0, nullptr, P(0x6000000), 1u << 30, 0, nullptr) == NCAHIP_EINVAL && said("epoch"));
        EXPECT(ncahip_dynca_clip_f32(PF(st), PF(gray), P(before + 1), fmt, 3, 2, 4, nullptr, PF(0x4000000), PF(0x4100000), PF(0x4200000), PF(0x4300000), 1, 12,
                                     3, 8, 8, 96, 1, 0, 0.5f, 0, 0, nullptr, P(0x6000000), 1u << 30, 0, nullptr) == NCAHIP_EINVAL && said("overlap"));
        EXPECT(ncahip_dynca_clip_xc_f32(PF(st), PF(gray), nullptr, 0, P(before), fmt, 3, 2, 4, nullptr, PF(0x4000000), PF(0x4100000), PF(0x4200000),
                                        PF(0x4300000), 1, 13, 3, 8, 8, 96, 1, 0, 0.5f, 0, 0, nullptr, P(0x6000000), 1u << 30, 0, nullptr) == NCAHIP_EINVAL && said("epoch"));
        EXPECT(ncahip_cond_clip_f32(PF(st), static_cast<uint8_t*>(P(0x5000000)), PF(gray), 12, P(before), fmt, 3, 2, 4, nullptr, PF(0x4000000), PF(0x4100000),
                                    PF(0x4200000), PF(0x4300000), PF(0x4400000), PF(0x4500000), 1, 16, 8, 8, 64, 3, 0.1f, 0.5f, -10.0f, 10.0f, 0, 0, P(0x6000000),
                                    1u << 30, 0, nullptr) == NCAHIP_EINVAL && said("epoch"));
        // as a frame format the same values stay unknown
        EXPECT(ncahip_clip_cond(P(0x100000), fmt, PF(0x200000), 0.3f, 0.3f, 0.3f, 1, PF(0x300000), 2, 1, 8, 8, nullptr) == NCAHIP_EINVAL && said("format"));
        EXPECT(ncahip_clip_gray(P(0x100000), fmt, 0.3f, 0.3f, 0.3f, PF(0x300000), 2, 1, 8, 8, nullptr) == NCAHIP_EINVAL && said("format"));
    }
    for (int fmt : {2, 7, -1, 0x108, 0xff})
        EXPECT(ncahip_clip_emit(PF(st), P(img), fmt, 1, 12, 3, 8, 8, nullptr) == NCAHIP_EINVAL && said("format"));
    std::printf(failures ? "host checks: %d FAILED\n" : "host checks of the planar image output: ok\n", failures);
    return failures ? 1 : 0;
}
