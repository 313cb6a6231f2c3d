// Exercises getDisparity_SGBM_census of include/aswMethods_mi355x.hpp (plain asw::Mat, or -DASW_WITH_OPENCV against
// tests/cpp/cv_stub):
//   sgbm_census_demo <H> <W> <C> <left.raw> <right.raw> <win> <minD> <numD> <paths> <out_u8.raw>
// Reads two 8U images of C channels, calls getDisparity_SGBM_census with `paths` and getDisparity_SGBM_paths with the same mask,
// writes the former and prints whether the two maps are the same (they should not be: another cost).  A throwing case prints
// "error".
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
    if (argc != 11) { fprintf(stderr, "usage\n"); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), C = atoi(argv[3]), win = atoi(argv[6]), minD = atoi(argv[7]), numD = atoi(argv[8]);
    const int paths = (int)strtol(argv[9], nullptr, 0);
    AswMat L = asw::detail::make(H, W, ASW_8U, C), R = asw::detail::make(H, W, ASW_8U, C), a, b;
    if (!read_file(argv[4], L.data, (size_t)H * W * C) || !read_file(argv[5], R.data, (size_t)H * W * C)) return 3;
    try {
        getDisparity_SGBM_census(L, R, a, win, minD, numD, paths);
        getDisparity_SGBM_paths(L, R, b, win, minD, numD, paths);
    } catch (const std::runtime_error& e) {
        printf("error %s\n", e.what());
        return 0;
    }
    const asw_image ai = asw::detail::view(a), bi = asw::detail::view(b);
    if (ai.depth != ASW_8U || ai.rows != H || ai.cols != W || ai.channels != 1) { printf("bad type\n"); return 4; }
    int same = 1;
    for (int y = 0; y < H; y++)
        same &= memcmp((const uint8_t*)ai.data + (size_t)y * ai.step, (const uint8_t*)bi.data + (size_t)y * bi.step, (size_t)W) == 0;
    FILE* f = fopen(argv[10], "wb");
    for (int y = 0; y < H; y++) fwrite((const uint8_t*)ai.data + (size_t)y * ai.step, 1, (size_t)W, f);
    fclose(f);
    printf("ok %d %d bt_same=%d\n", H, W, same);
    return 0;
}
