// enlarge_check.cpp -- csrc/kbe_enlarge_block.h compiled by g++ and executed serially: the definition of kbe_enlarge_u8
// (tests/test_enlarge_stream.py).  Build: g++ -O2 -std=c++17 -fsanitize=signed-integer-overflow,address -fno-sanitize-recover=all -I csrc
// (no -ffast-math, no -march); a plain program, run as it is.
//
//   enlarge_check brute MAX
//       every n_in <= n_out <= MAX and every x: taps() against the weights as exact rationals in __int128 -- the position i + r / D by
//       i D <= p < (i + 1) D, each of c0, c2, c3 by c 2 D^3 <= n 16384 + D^3 < (c + 1) 2 D^3 with n from a Horner form of its own (a floor
//       is that, also of a negative numerator), the sum 16384, the taps i - 1 .. i + 2 clamped; and at n_out == n_in (0, 16384, 0, 0).
//   enlarge_check limits
//       every x of 16383 -> 16384, 1 -> 16384 and 16384 -> 16384, the same way: the worst cases of the int64 bound, under the sanitizer.
//   enlarge_check enlarge W H stride cw ch w h n in.raw out.raw
//       in.raw: n frames [H][stride] bytes back to back; out.raw: n frames [h][w][3].
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kbe_enlarge_block.h"

using namespace kbe_enlarge;
typedef __int128 wide;

struct Tally {
    long axes = 0, indices = 0, bad_positions = 0, bad_floors = 0, bad_sums = 0, bad_taps = 0, bad_identities = 0, negative = 0;
    int lowest = 1 << 30, highest = -(1 << 30);
    bool bad() const { return bad_positions || bad_floors || bad_sums || bad_taps || bad_identities; }
};

static void check_axis(uint32_t n_in, uint32_t n_out, Tally& t)
{
    t.axes++;
    const wide D = 2 * (wide) n_out, den = 2 * D * D * D;
    for (uint32_t x = 0; x < n_out; x++) {
        t.indices++;
        const Taps a = taps(n_in, n_out, x);
        uint32_t r32;
        const int32_t i = position(n_in, n_out, x, &r32);
        const wide p = (2 * (wide) x + 1) * n_in - n_out, r = r32;
        if (!((wide) i * D <= p && p < ((wide) i + 1) * D && r == p - (wide) i * D)) t.bad_positions++;
        // the numerators over 2 D^3, by Horner in r
        const wide n[4] = {((-r + 2 * D) * r - D * D) * r, (3 * r - 5 * D) * r * r + den, ((-3 * r + 4 * D) * r + D * D) * r, (r - D) * r * r};
        if (n[0] + n[1] + n[2] + n[3] != den) t.bad_sums++;                 // (the weights themselves add up to 1)
        for (int k = 0; k < 4; k++) {
            if (k != 1 && !((wide) a.c[k] * den <= n[k] * kOne + D * D * D && n[k] * kOne + D * D * D < ((wide) a.c[k] + 1) * den)) t.bad_floors++;
            if (a.c[k] < 0) t.negative++;
            if (a.c[k] < t.lowest) t.lowest = a.c[k];
            if (a.c[k] > t.highest) t.highest = a.c[k];
            const int32_t tap = i - 1 + k, want = tap < 0 ? 0 : tap > (int32_t) n_in - 1 ? (int32_t) n_in - 1 : tap;
            if (a.t[k] != (uint32_t) want) t.bad_taps++;
        }
        if (a.c[0] + a.c[1] + a.c[2] + a.c[3] != kOne) t.bad_sums++;
        if (n_in == n_out && !(a.c[0] == 0 && a.c[1] == kOne && a.c[2] == 0 && a.c[3] == 0 && a.t[1] == x)) t.bad_identities++;
    }
}

static int report(const char* what, const Tally& t)
{
    printf("%s: axes %ld, indices %ld, bad positions %ld, bad floors %ld, bad sums %ld, bad taps %ld, bad identities %ld, negative %ld, lowest %d, highest %d\n", what, t.axes, t.indices,
           t.bad_positions, t.bad_floors, t.bad_sums, t.bad_taps, t.bad_identities, t.negative, t.lowest, t.highest);
    return t.bad();
}

static int brute(int max_side)
{
    Tally t;
    for (uint32_t n_out = 1; n_out <= (uint32_t) max_side; n_out++)
        for (uint32_t n_in = 1; n_in <= n_out; n_in++) check_axis(n_in, n_out, t);
    return report("brute", t);
}

static int limits()
{
    Tally t;
    check_axis(kMaxOut - 1, kMaxOut, t);
    check_axis(1, kMaxOut, t);
    check_axis(kMaxOut, kMaxOut, t);
    return report("limits", t);
}

static int run(char** argv)
{
    const int W = atoi(argv[2]), H = atoi(argv[3]), stride = atoi(argv[4]), cw = atoi(argv[5]), ch = atoi(argv[6]), w = atoi(argv[7]), h = atoi(argv[8]), n = atoi(argv[9]);
    if (!shape_ok(W, H, cw, ch, w, h) || stride < 3 * W || n < 1) { fprintf(stderr, "refused\n"); return 2; }
    std::vector<uint8_t> src((size_t) n * H * stride), out((size_t) n * h * w * 3);
    FILE* f = fopen(argv[10], "rb");
    const bool read = f && fread(src.data(), 1, src.size(), f) == src.size();
    if (f) fclose(f);
    if (!read) { fprintf(stderr, "cannot read %s\n", argv[10]); return 2; }
    const Crop k = {(uint32_t) W, (uint32_t) H, (uint32_t) cw, (uint32_t) ch};
    for (int i = 0; i < n; i++)
        for (uint32_t oy = 0; oy < (uint32_t) h; oy++)
            for (uint32_t ox = 0; ox < (uint32_t) w; ox++)
                enlarge_pixel(k, (uint32_t) w, (uint32_t) h, src.data() + (size_t) i * H * stride, (size_t) stride, ox, oy, &out[(((size_t) i * h + oy) * w + ox) * 3]);
    f = fopen(argv[11], "wb");
    const bool written = f && fwrite(out.data(), 1, out.size(), f) == out.size();
    if (f) fclose(f);
    if (!written) { fprintf(stderr, "cannot write %s\n", argv[11]); return 2; }
    printf("enlarged %d frames %dx%d, crop %dx%d -> %dx%d\n", n, W, H, cw, ch, w, h);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "brute")) return brute(atoi(argv[2]));
    if (argc == 2 && !strcmp(argv[1], "limits")) return limits();
    if (argc == 12 && !strcmp(argv[1], "enlarge")) return run(argv);
    fprintf(stderr, "usage: enlarge_check brute MAX | limits | enlarge W H stride cw ch w h n in.raw out.raw\n");
    return 2;
}
