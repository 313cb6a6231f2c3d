// Exercises the refinement half of include/aswMethods_mi355x.hpp (plain asw::Mat, or -DASW_WITH_OPENCV against tests/cpp/cv_stub):
//   refine_demo <H> <W> <C> <left.raw> <right.raw> <alg> <win> <minD> <numD> <maxDiff> <refineWin> <gamma_c> <gamma_s> <one_call.raw> <blocks.raw>
// Reads two 8U images of C channels; writes the f32 map of stereoMatchingRefined and the one refineDisparity makes of two plain
// stereoMatching results.  A status the shim throws on prints "error".
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
    if (argc != 16) { fprintf(stderr, "usage\n"); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), C = atoi(argv[3]), alg = atoi(argv[6]), win = atoi(argv[7]), minD = atoi(argv[8]),
              numD = atoi(argv[9]), rwin = atoi(argv[11]);
    const float maxDiff = (float)atof(argv[10]);
    const double gc = atof(argv[12]), gs = atof(argv[13]);
    AswMat L = asw::detail::make(H, W, ASW_8U, C), R = asw::detail::make(H, W, ASW_8U, C), dl, dr;
    if (!read_file(argv[4], L.data, (size_t)H * W * C) || !read_file(argv[5], R.data, (size_t)H * W * C)) return 3;
    int rej1 = -1, unf1 = -1, rej2 = -1, unf2 = -1;
    try {
        AswMat one = stereoMatchingRefined(L, R, (StereoMatchingAlgorithms)alg, win, minD, numD, maxDiff, rwin, gc, gs, &rej1, &unf1);
        stereoMatching(L, R, dl, DISPARITY_LEFT, (StereoMatchingAlgorithms)alg, win, minD, numD);
        stereoMatching(L, R, dr, DISPARITY_RIGHT, (StereoMatchingAlgorithms)alg, win, minD, numD);
        AswMat two = refineDisparity(L, dl, dr, minD, asw_volume_planes(alg, numD), maxDiff, rwin, gc, gs, &rej2, &unf2);
        if (!write_map(argv[14], one, H, W) || !write_map(argv[15], two, H, W)) { printf("bad type\n"); return 4; }
    } catch (const std::runtime_error& e) {
        printf("error %s\n", e.what());
        return 0;
    }
    printf("ok %d %d rejected=%d,%d unfillable=%d,%d\n", H, W, rej1, rej2, unf1, unf2);
    return 0;
}
