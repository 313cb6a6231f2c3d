// Exercises the BM half of include/aswMethods_mi355x.hpp (plain asw::Mat, or -DASW_WITH_OPENCV against tests/cpp/cv_stub):
//   bm_demo <H> <W> <C> <left.raw> <right.raw> <win> <minD> <numD> <out_u8.raw>
// Reads two 8U images of C channels, calls getDisparity_BM (M.h:93) and writes its CV_8U map; checks that the selector's BM entry
// still throws.  A CV_Error case of the reference prints "error".
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
    if (argc != 10) { fprintf(stderr, "usage\n"); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), C = atoi(argv[3]), win = atoi(argv[6]), minD = atoi(argv[7]), numD = atoi(argv[8]);
    AswMat L = asw::detail::make(H, W, ASW_8U, C), R = asw::detail::make(H, W, ASW_8U, C), a, b;
    if (!read_file(argv[4], L.data, (size_t)H * W * C) || !read_file(argv[5], R.data, (size_t)H * W * C)) return 3;
    try {
        getDisparity_BM(L, R, a, win, minD, numD);
    } catch (const std::runtime_error& e) {
        printf("error %s\n", e.what());
        return 0;
    }
    int selector_throws = 0;
    try {
        stereoMatching(L, R, b, DISPARITY_LEFT, BM, win, minD, numD);
    } catch (const std::runtime_error&) {
        selector_throws = 1;
    }
    const asw_image ai = asw::detail::view(a);
    if (ai.depth != ASW_8U || ai.channels != 1 || ai.rows != H || ai.cols != W) { printf("bad type\n"); return 4; }
    FILE* f = fopen(argv[9], "wb");
    for (int y = 0; y < H; y++) fwrite((const uint8_t*)ai.data + (size_t)y * ai.step, 1, (size_t)W, f);
    fclose(f);
    printf("ok %d %d selector_throws=%d\n", H, W, selector_throws);
    return 0;
}
