// rows_check.cpp -- csrc/kbe_rows.h compiled by g++ and executed serially: how the frame filters fetch and store a row of 3-byte pixels, held
// to the bytes themselves (tests/test_filter_sweeps.py).  Build: g++ -O2 -std=c++17 -I csrc (no -ffast-math, no -march).
//
//   rows_check brute
//       store_piece over a row of every length from 1 to 80 bytes at every lead from 0 to 15, into a buffer of 0x5A with bands on both sides:
//       every call changes exactly the bytes of its piece that the row has, to the piece's own, so every byte of the row is written exactly
//       once and nothing else changes; piece_of's bounds, whole() and dword_is_whole() against the definition by brute force, and how many
//       pieces, dwords and bytes go which way (the test counts them again);
//       lead_of and store_tile_row at real addresses: tiles of 1..64 pixels at every lead, the LDS row a 16-byte aligned buffer;
//       fetch_of at every shift and rows of 1..40 pixels: the aligned dwords hold the row, every one of them a byte of it, `shift` bytes in;
//       realign<N> for N = 4, 6 and 12 at b = 0..3 against the bytes themselves;
//       dword_holds_a_byte<N> and all_dwords_hold_a_byte<N> (N = 4 on long, N = 12 on int) against the definition by brute force, for rows of
//       1..40 bytes and j0 from -19 to 3 past the row's end.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "kbe_rows.h"

using namespace kbe_rows;

static long piece_bad = 0, pieces = 0, sixteens = 0, dword_stores = 0, byte_stores = 0;

// one row of n bytes, `lead` bytes into its first piece
static void store_row(long n, uint32_t lead)
{
    const long band = 32, size = band + 16 + n + 16 + band;
    std::vector<uint8_t> buf(size, 0x5A), before;
    std::vector<int> written(size, 0);
    uint8_t* const row = buf.data() + band + lead;                             // (buf + band stands for an address that is a multiple of 16)
    const uint32_t end = lead + (uint32_t) n;
    for (uint32_t at = 0; at < end; at += kPiece, pieces++) {
        // the definition: byte i of the piece is byte at + i - lead of the row, if the row has it
        bool mine[16];
        uint32_t lo = 16u, hi = 0u;
        for (uint32_t i = 0; i < 16u; i++) {
            mine[i] = at + i >= lead && at + i < end;
            if (mine[i]) lo = i < lo ? i : lo, hi = i + 1u;
        }
        const Piece q = piece_of(row, lead, end, at);
        if (q.p != buf.data() + band + at || q.lo != lo || q.hi != hi) piece_bad++;
        bool all = true;
        for (uint32_t i = 0; i < 16u; i++) all = all && mine[i];
        if (q.whole() != all) piece_bad++;
        for (uint32_t d = 0; d < 4u; d++) {
            const bool four = mine[4u * d] && mine[4u * d + 1u] && mine[4u * d + 2u] && mine[4u * d + 3u];
            if (dword_is_whole(q, d) != four) piece_bad++;
            if (all) continue;
            if (four) dword_stores++;
            else
                for (uint32_t i = 4u * d; i < 4u * d + 4u; i++) byte_stores += mine[i] ? 1 : 0;
        }
        sixteens += all ? 1 : 0;
        // two stores, the second of the first's bytes flipped: no byte of either is 0x5A, so every byte written shows in one of them
        // (1..64 and their complements)
        for (int turn = 0; turn < 2; turn++) {
            uint8_t bytes[16];
            uint32_t word[4];
            for (uint32_t i = 0; i < 16u; i++) bytes[i] = (uint8_t) (turn ? ~(1u + (i + at) % 64u) : 1u + (i + at) % 64u);
            memcpy(word, bytes, 16);
            before = buf;
            store_piece(row, lead, end, at, word);
            for (long k = 0; k < size; k++) {
                const long i = k - band - (long) at;                           // as a byte of the piece
                const bool in = i >= 0 && i < 16 && mine[i];
                if (in ? buf[k] != bytes[i] : buf[k] != before[k]) piece_bad++;
                if (in && turn == 0) written[k]++;
            }
        }
    }
    for (long k = 0; k < size; k++) {
        const bool in = k >= band + (long) lead && k < band + (long) lead + n;
        if (written[k] != (in ? 1 : 0) || (!in && buf[k] != 0x5A)) piece_bad++;
    }
}

// a tile's row of nx pixels through its LDS row, at a real address `lead` bytes beyond a multiple of 16
static long tile_row_bad(uint32_t nx, uint32_t lead)
{
    alignas(16) uint8_t lds[3 * 64 + 16], memory[32 + 16 + 3 * 64 + 16 + 32];
    long bad = 0;
    memset(lds, 0xA5, sizeof(lds));
    memset(memory, 0x5A, sizeof(memory));
    uint8_t* const row = memory + 32 + lead;
    if (lead_of(row) != lead) bad++;
    for (uint32_t b = 0; b < 3u * nx; b++) lds[lead_of(row) + b] = (uint8_t) (1u + b % 89u);
    for (uint32_t lane = 0; lane < 13u; lane++) store_tile_row(lds, row, nx, 16u * lane);
    for (long k = 0; k < (long) sizeof(memory); k++) {
        const long b = k - 32 - (long) lead;
        if (memory[k] != (b >= 0 && b < 3l * nx ? (uint8_t) (1 + b % 89) : (uint8_t) 0x5A)) bad++;
    }
    return bad;
}

static long fetch_bad(uint32_t n, uint32_t shift)
{
    alignas(16) uint8_t memory[16 + 4 + 3 * 40 + 4];
    for (size_t k = 0; k < sizeof(memory); k++) memory[k] = (uint8_t) (3 * k + 1);
    const uint8_t* const first = memory + 16 + shift;
    const Fetch f = fetch_of(first, n);
    long bad = 0;
    if (f.shift != shift || shift_of(first) != shift || (const uint8_t*) f.base != memory + 16) bad++;
    // the fewest dwords that hold the row: the last of them holds a byte of it
    if (4u * f.dwords < shift + 3u * n || 4u * (f.dwords - 1u) >= shift + 3u * n) bad++;
    uint32_t copy[32];
    memcpy(copy, f.base, 4u * f.dwords);
    if (memcmp((const uint8_t*) copy + f.shift, first, 3u * n) != 0) bad++;
    return bad;
}

template <int N>
static long realign_bad()
{
    long bad = 0;
    for (uint32_t b = 0; b < 4u; b++) {
        uint8_t bytes[4 * (N + 1)], got[4 * N];
        for (int i = 0; i < 4 * (N + 1); i++) bytes[i] = (uint8_t) (17 * i + 3);
        uint32_t x[N + 1], w[N];
        memcpy(x, bytes, sizeof(bytes));
        realign<N>(x, b, w);
        memcpy(got, w, sizeof(got));
        if (memcmp(got, bytes + b, sizeof(got)) != 0) bad++;
    }
    return bad;
}

// The definition: dword k of the N + 1 covers the bytes j0 - b + 4 k .. + 3 of the row.  It is loaded if one of them is a byte of the row
// and one of them is among the 4 N bytes wanted, j0 .. j0 + 4 N - 1; all of them are loaded at once where every one holds a byte of the row
// at every b.
template <int N, class Int>
static long rule_bad(long* asked)
{
    long bad = 0;
    for (Int n = 1; n <= 40; n++)
        for (Int j0 = -19; j0 <= n + 3; j0++) {
            bool every = true;
            for (uint32_t b = 0; b < 4u; b++)
                for (int k = 0; k <= N; k++, (*asked)++) {
                    bool holds = false, wanted = false;
                    for (Int i = 0; i < 4; i++) {
                        const Int j = j0 - (Int) b + 4 * k + i;
                        holds = holds || (j >= 0 && j < n);
                        wanted = wanted || (j >= j0 && j < j0 + 4 * N);
                    }
                    every = every && holds;
                    if (dword_holds_a_byte<N>(j0, b, k, n) != (holds && wanted)) bad++;
                }
            if (all_dwords_hold_a_byte<N>(j0, n) != every) bad++;
        }
    return bad;
}

static int brute()
{
    for (long n = 1; n <= 80; n++)
        for (uint32_t lead = 0; lead < 16u; lead++) store_row(n, lead);
    long tile_rows = 0, tile_bad = 0, fetches = 0, fetches_bad = 0, asked = 0;
    for (uint32_t nx = 1; nx <= 64u; nx++)
        for (uint32_t lead = 0; lead < 16u; lead++, tile_rows++) tile_bad += tile_row_bad(nx, lead);
    for (uint32_t n = 1; n <= 40u; n++)
        for (uint32_t shift = 0; shift < 4u; shift++, fetches++) fetches_bad += fetch_bad(n, shift);
    const long realigned_bad = realign_bad<4>() + realign_bad<6>() + realign_bad<12>();
    const long rules_bad = rule_bad<4, long>(&asked) + rule_bad<12, int>(&asked);
    printf("brute: pieces %ld, piece mismatches %ld, whole pieces %ld, dwords %ld, bytes %ld, tile rows %ld, tile row mismatches %ld, fetches %ld, fetch mismatches %ld, "
           "realign mismatches %ld, dwords asked %ld, dword rule mismatches %ld\n",
           pieces, piece_bad, sixteens, dword_stores, byte_stores, tile_rows, tile_bad, fetches, fetches_bad, realigned_bad, asked, rules_bad);
    return piece_bad || tile_bad || fetches_bad || realigned_bad || rules_bad ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "brute")) return brute();
    fprintf(stderr, "usage: rows_check brute\n");
    return 2;
}
