// Exercises stereoMatchingScanline of include/aswMethods_mi355x.hpp (plain asw::Mat, or -DASW_WITH_OPENCV against tests/cpp/cv_stub):
//   scanline_demo <H> <W> <C> <left.raw> <right.raw> <type> <alg> <win> <minD> <numD> <p1_code> <unit_code> <p2_ratio> <subpixel> <shim.raw> <c_abi.raw>
// Reads two 8U images of C channels; writes the f32 map of the shim call and the one of asw_stereo_match with
// asw_disparity_scanline() OR-ed into disparity_type.  A status the shim throws on prints "error".
#include <cstdio>
#include <cstdlib>
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
    if (argc != 17) { fprintf(stderr, "usage\n"); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), C = atoi(argv[3]), type = atoi(argv[6]), alg = atoi(argv[7]), win = atoi(argv[8]),
              minD = atoi(argv[9]), numD = atoi(argv[10]), a = atoi(argv[11]), u = atoi(argv[12]), ratio = atoi(argv[13]), sub = atoi(argv[14]);
    AswMat L = asw::detail::make(H, W, ASW_8U, C), R = asw::detail::make(H, W, ASW_8U, C), shim;
    if (!read_file(argv[4], L.data, (size_t)H * W * C) || !read_file(argv[5], R.data, (size_t)H * W * C)) return 3;
    try {
        stereoMatchingScanline(L, R, shim, (DisparityType)type, (StereoMatchingAlgorithms)alg, win, minD, numD, a, u, ratio, sub);
    } catch (const std::runtime_error& e) {
        printf("error %s\n", e.what());
        return 0;
    }
    AswMat plain = asw::detail::make(H, W, ASW_32F, 1);
    asw_image li = asw::detail::view(L), ri = asw::detail::view(R), di = asw::detail::view(plain);
    const int rc = asw_stereo_match(asw::detail::context(), &li, &ri, &di, type | sub | asw_disparity_scanline(a, u, ratio), alg, win, minD,
                                    numD, nullptr, 0);
    if (rc != ASW_OK) { printf("status %d\n", rc); return 5; }
    if (!write_map(argv[15], shim, H, W) || !write_map(argv[16], plain, H, W)) { printf("bad type\n"); return 4; }
    printf("ok %d %d\n", H, W);
    return 0;
}
