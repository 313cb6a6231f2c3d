// Exercises computeAdaptiveWeight_permeability of include/aswMethods_mi355x.hpp (plain asw::Mat, or -DASW_WITH_OPENCV against
// tests/cpp/cv_stub):
//   permeability_demo <H> <W> <C> <left.raw> <right.raw> <right_view 0|1> <sigma> <trunc> <minD> <numD> <out_f32.raw>
// Reads two 8U images of C channels, calls the wrapper, and checks whether asw_stereo_match gives the same map with the value
// asw_alg_permeability forms from the call's own parameters (the table cache is keyed by sigma) and an even window: the method has
// none.  A throwing case prints "error".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "aswMethods_mi355x.hpp"

static bool read_file(const char* path, void* dst, size_t n)
{
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    size_t got = fread(dst, 1, n, f);
    fclose(f);
    return got == n;
}

int main(int argc, char** argv)
{
    if (argc != 12) { fprintf(stderr, "usage\n"); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), C = atoi(argv[3]), right = atoi(argv[6]);
    const int sigma = atoi(argv[7]), trunc = atoi(argv[8]), minD = atoi(argv[9]), numD = atoi(argv[10]);
    const DisparityType dt = right ? DISPARITY_RIGHT : DISPARITY_LEFT;
    AswMat L = asw::detail::make(H, W, ASW_8U, C), R = asw::detail::make(H, W, ASW_8U, C), a, b;
    if (!read_file(argv[4], L.data, (size_t)H * W * C) || !read_file(argv[5], R.data, (size_t)H * W * C)) return 3;
    try {
        a = computeAdaptiveWeight_permeability(L, R, dt, sigma, trunc, minD, numD);
        if (!a.empty()) {
            asw_image li = asw::detail::view(L), ri = asw::detail::view(R);
            b = asw::detail::make(H, W, ASW_32F, 1);
            asw_image bi = asw::detail::view(b);
            const int rc = asw_stereo_match(asw::detail::context(), &li, &ri, &bi, (int)dt, asw_alg_permeability(sigma, trunc), 16, minD,
                                            numD, nullptr, 0);
            if (rc != ASW_OK) { printf("selector status %d\n", rc); return 5; }
        }
    } catch (const std::runtime_error& e) {
        printf("error %s\n", e.what());
        return 0;
    }
    if (a.empty()) { printf("empty\n"); return 0; }
    const asw_image ai = asw::detail::view(a), bi = asw::detail::view(b);
    if (ai.depth != ASW_32F || ai.rows != H || ai.cols != W || ai.channels != 1) { printf("bad type\n"); return 4; }
    int same = 1;
    for (int y = 0; y < H; y++)
        same &= memcmp((const uint8_t*)ai.data + (size_t)y * ai.step, (const uint8_t*)bi.data + (size_t)y * bi.step, (size_t)W * 4) == 0;
    FILE* f = fopen(argv[11], "wb");
    for (int y = 0; y < H; y++) fwrite((const uint8_t*)ai.data + (size_t)y * ai.step, 4, (size_t)W, f);
    fclose(f);
    printf("ok %d %d selector_same=%d\n", H, W, same);
    return 0;
}
