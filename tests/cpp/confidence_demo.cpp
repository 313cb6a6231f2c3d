// Exercises stereoMatchingConfidence of include/aswMethods_mi355x.hpp (plain asw::Mat, or -DASW_WITH_OPENCV against tests/cpp/cv_stub):
//   confidence_demo <H> <W> <C> <left.raw> <right.raw> <type> <alg> <win> <minD> <numD> <shim_disp.raw> <shim_conf.raw> <c_abi.raw>
// Reads two 8U images of C channels; <type> may carry the flags of disparity_type.  Writes the two f32 maps of the shim call and the
// interleaved 2-channel f32 image of asw_stereo_match, with 3 floats of padding per row.  A status the shim throws on prints "error";
// a silent status (two empty Mats) prints "empty".
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

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
    if (argc != 14) { fprintf(stderr, "usage\n"); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), C = atoi(argv[3]), type = atoi(argv[6]), alg = atoi(argv[7]), win = atoi(argv[8]),
              minD = atoi(argv[9]), numD = atoi(argv[10]);
    AswMat L = asw::detail::make(H, W, ASW_8U, C), R = asw::detail::make(H, W, ASW_8U, C), disp, conf;
    if (!read_file(argv[4], L.data, (size_t)H * W * C) || !read_file(argv[5], R.data, (size_t)H * W * C)) return 3;
    try {
        stereoMatchingConfidence(L, R, disp, conf, type, (StereoMatchingAlgorithms)alg, win, minD, numD);
    } catch (const std::runtime_error& e) {
        printf("error %s\n", e.what());
        return 0;
    }
    if (disp.empty() && conf.empty()) { printf("empty\n"); return 0; }
    const size_t row = (size_t)W * 2 + 3;  // floats per row of the C-ABI call's image: padded
    std::vector<float> both(row * H, -7.5f);
    asw_image li = asw::detail::view(L), ri = asw::detail::view(R);
    asw_image bi{both.data(), H, W, 2, ASW_32F, row * sizeof(float)};
    const int rc = asw_stereo_match(asw::detail::context(), &li, &ri, &bi, type, alg, win, minD, numD, nullptr, 0);
    if (rc != ASW_OK) { printf("status %d\n", rc); return 5; }
    if (!write_map(argv[11], disp, H, W) || !write_map(argv[12], conf, H, W)) { printf("bad type\n"); return 4; }
    FILE* f = fopen(argv[13], "wb");
    if (!f) return 4;
    fwrite(both.data(), sizeof(float), both.size(), f);
    fclose(f);
    printf("ok %d %d\n", H, W);
    return 0;
}
