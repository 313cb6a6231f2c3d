// The two word decoders of csrc/asw_selector.h as a filter: case lines on stdin, one result line per case on stdout
// (tests/test_selector_words_cpu.py holds the output to the record under tests/golden/).  No library, no GPU.
//   A <word> <null_mp>               decode_algorithm(word, &method, null_mp ? nullptr : &mp, traits)
//   D <word> <traits> <minD> <numD>  decode_disparity_type(m, served, 1025, mp) with mp = match_params(word, 5, minD, numD)
// <word>: 8 hex digits.  <traits>: -1 = a value outside the table (m null), else bit 0 served, bit 1 no_volume, bit 2
// ignores_disparity_type, bit 3 no_subpixel, bit 4 extra_planes = 1.
// A refused D case prints its status alone: run_method decodes into a copy of its own, so nothing else of it can be seen.
#include <stdio.h>

#include "asw_selector.h"

// the selector values as decode_algorithm needs them: 0..12 exist, 12 takes packed parameters
static const MethodTraits* traits(int method)
{
    static const MethodTraits plain = {0, false, false, false, false}, packed = {0, false, false, false, true};
    return method < 0 || method > ASW_ALG_ADAPTIVE_WEIGHT_CROSS ? nullptr : method == ASW_ALG_ADAPTIVE_WEIGHT_CROSS ? &packed : &plain;
}

static void case_algorithm(unsigned word, int null_mp)
{
    MatchParams mp = match_params(0, 5, 0, 1);
    int method = -1;
    const int rc = decode_algorithm((int)word, &method, null_mp ? nullptr : &mp, traits);
    printf("A %08x %d -> %d %d %d %g %g %d %d %d %d %d %d %d %d\n", word, null_mp, rc, method, mp.twopass, mp.gamma_c, mp.gamma_g,
           mp.cross_cost, mp.cross_tau, mp.cross_trunc, mp.lambda_ad, mp.lambda_census, mp.permeability, mp.perm_sigma, mp.perm_trunc);
}

static void case_disparity_type(unsigned word, int t, int minD, int numD)
{
    MatchParams mp = match_params((int)word, 5, minD, numD);
    const MethodTraits row = {(t >> 4) & 1, (t & 2) != 0, (t & 4) != 0, (t & 8) != 0, false};
    const int rc = decode_disparity_type(t < 0 ? nullptr : &row, t >= 0 && (t & 1), 1025, mp);
    printf("D %08x %d %d %d -> %d", word, t, minD, numD, rc);
    if (rc == ASW_OK)
        printf(" %08x %x %d %d %a %a", (unsigned)mp.disparity_type, (unsigned)mp.subpixel, mp.cross_scales, mp.cross_lambda_q, mp.scan_p1,
               mp.scan_p2);
    printf("\n");
}

int main()
{
    char kind;
    unsigned word;
    while (scanf(" %c %x", &kind, &word) == 2) {
        int a, b, c;
        if (kind == 'A' && scanf("%d", &a) == 1)
            case_algorithm(word, a);
        else if (kind == 'D' && scanf("%d %d %d", &a, &b, &c) == 3)
            case_disparity_type(word, a, b, c);
        else
            break;
    }
    return feof(stdin) ? 0 : 1;  // a line that is no case: the output is short, and the exit status says so
}
