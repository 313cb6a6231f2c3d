// Exercises the smoothing half of include/aswMethods_mi355x.hpp (plain asw::Mat, or -DASW_WITH_OPENCV against tests/cpp/cv_stub):
//   smooth_demo <H> <W> <C> <left.raw> <right.raw> <alg> <win> <minD> <numD> <sigma_c> <lambda> <iterations> <one_call.raw> <blocks.raw>
// Reads two 8U images of C channels; writes the f32 map of stereoMatchingSmoothed and the one smoothDisparity makes of the two maps
// of stereoMatchingConfidence.  A status the shim throws on prints "error", a silent one "empty".
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

static bool write_map(const char* path, const AswMat& m, int H, int W)
{
    const asw_image v = asw::detail::view(m);
    if (v.depth != ASW_32F || v.channels != 1 || v.rows != H || v.cols != W) return false;
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    for (int y = 0; y < H; y++) fwrite((const uint8_t*)v.data + (size_t)y * v.step, 4, (size_t)W, f);
    fclose(f);
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 15) { fprintf(stderr, "usage\n"); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), C = atoi(argv[3]), alg = atoi(argv[6]), win = atoi(argv[7]), minD = atoi(argv[8]),
              numD = atoi(argv[9]), T = atoi(argv[12]);
    const double sigma_c = atof(argv[10]), lambda = atof(argv[11]);
    AswMat L = asw::detail::make(H, W, ASW_8U, C), R = asw::detail::make(H, W, ASW_8U, C), d, c;
    if (!read_file(argv[4], L.data, (size_t)H * W * C) || !read_file(argv[5], R.data, (size_t)H * W * C)) return 3;
    try {
        AswMat one = stereoMatchingSmoothed(L, R, (StereoMatchingAlgorithms)alg, win, minD, numD, sigma_c, lambda, T);
        if (one.empty()) { printf("empty\n"); return 0; }
        stereoMatchingConfidence(L, R, d, c, DISPARITY_LEFT, (StereoMatchingAlgorithms)alg, win, minD, numD);
        AswMat two = smoothDisparity(L, d, c, sigma_c, lambda, T);
        if (!write_map(argv[13], one, H, W) || !write_map(argv[14], two, H, W)) { printf("bad type\n"); return 4; }
    } catch (const std::runtime_error& e) {
        printf("error %s\n", e.what());
        return 0;
    }
    printf("ok %d %d\n", H, W);
    return 0;
}
