// Exercises the per-method wrappers of include/aswMethods_mi355x.hpp whose parameters travel in the selector's algorithm value (plain
// asw::Mat, or -DASW_WITH_OPENCV against tests/cpp/cv_stub):
//   selector_demo cross    <H> <W> <C> <left.raw> <right.raw> <right_view 0|1> <tau> <trunc> <win> <minD> <numD> <out_f32.raw>
//   selector_demo adcensus <H> <W> <C> <left.raw> <right.raw> <right_view 0|1> <tau> <lambda_ad> <lambda_census> <win> <minD> <numD> <out_f32.raw>
//   selector_demo twopass  <H> <W> <C> <left.raw> <right.raw> <right_view 0|1> <gamma_c> <gamma_g> <win> <minD> <numD> <out_f32.raw>
// Reads two 8U images of C channels, calls computeAdaptiveWeight_<method>, and checks whether asw_stereo_match gives the same map with
// the value asw_alg_<method> forms: from the defaults for cross (20, 20) and adcensus (20, 10, 30), so that other parameters show as
// selector_same=0, and from the call's own gammas for twopass, whose table cache is keyed by them.  An even window prints "empty", a
// throwing case "error".
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
    static const char* const names[3] = {"cross", "adcensus", "twopass"};
    static const int counts[3] = {2, 3, 2};
    int m = 0;
    while (m < 3 && (argc < 2 || strcmp(argv[1], names[m]))) m++;
    if (m == 3 || argc != 12 + counts[m]) { fprintf(stderr, "usage\n"); return 2; }
    const int H = atoi(argv[2]), W = atoi(argv[3]), C = atoi(argv[4]), right = atoi(argv[7]);
    int p[3] = {0, 0, 0};
    for (int i = 0; i < counts[m]; i++) p[i] = atoi(argv[8 + i]);
    char** rest = argv + 8 + counts[m];
    const int win = atoi(rest[0]), minD = atoi(rest[1]), numD = atoi(rest[2]);
    const DisparityType dt = right ? DISPARITY_RIGHT : DISPARITY_LEFT;
    AswMat L = asw::detail::make(H, W, ASW_8U, C), R = asw::detail::make(H, W, ASW_8U, C), a, b;
    if (!read_file(argv[5], L.data, (size_t)H * W * C) || !read_file(argv[6], R.data, (size_t)H * W * C)) return 3;
    try {
        a = m == 0 ? computeAdaptiveWeight_cross(L, R, dt, p[0], p[1], win, minD, numD)
          : m == 1 ? computeAdaptiveWeight_adcensus(L, R, dt, p[0], p[1], p[2], win, minD, numD)
                   : computeAdaptiveWeight_twopass(L, R, p[0], p[1], dt, win, minD, numD);
        if (!a.empty()) {
            const int alg = m == 0 ? asw_alg_cross(20, 20) : m == 1 ? asw_alg_adcensus(20, 10, 30) : asw_alg_twopass(p[0], p[1]);
            asw_image li = asw::detail::view(L), ri = asw::detail::view(R);
            b = asw::detail::make(H, W, ASW_32F, 1);
            asw_image bi = asw::detail::view(b);
            const int rc = asw_stereo_match(asw::detail::context(), &li, &ri, &bi, (int)dt, alg, win, minD, numD, nullptr, 0);
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
    FILE* f = fopen(rest[3], "wb");
    for (int y = 0; y < H; y++) fwrite((const uint8_t*)ai.data + (size_t)y * ai.step, 4, (size_t)W, f);
    fclose(f);
    printf("ok %d %d selector_same=%d\n", H, W, same);
    return 0;
}
