// Steps the row-leaf body of the Merkle row commitment (merkle_row_leaf_at, toyni_amd/csrc/merkle_kernels.hpp) on the CPU.
// For every width 1 .. max_width (argv[1], default 40), salted and unsalted, both layouts (column-major with a padded column
// stride, row-major with word loads and -- where the width allows -- 16-byte loads) it hashes ROWS rows and prints one line per leaf:
//     <width> <salted> <layout> <vec> <blocks> <leaf bytes as hex> <digest as hex>
// tests/test_emu_rows.py recomputes sha256(00 || leaf) with hashlib.  The matrices are allocated with exactly the words the layout
// owns (the slack between n and col_stride excluded at the end), so an over-read is an AddressSanitizer error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>

#include "merkle_kernels.hpp"

using namespace toyni;

static uint64_t sm_state = 0x9E3779B97F4A7C15ull;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t draw_value(uint32_t row, uint32_t col) {
    const uint32_t P = 2013265921u;
    switch ((row + col) % 4) {      // {0, 1, p - 1, random}
        case 0: return 0u;
        case 1: return 1u;
        case 2: return P - 1u;
        default: return (uint32_t)(splitmix() % P);
    }
}
static void hex(const uint8_t* b, size_t n) {
    for (size_t i = 0; i < n; ++i) std::printf("%02x", b[i]);
}

template <int LAYOUT, bool SALTED>
static void run(uint32_t width, bool vec, const std::vector<uint32_t>& rows /* row-major ROWS x width */, uint32_t nrows,
                const std::vector<uint8_t>& salts) {
    const uint64_t col_stride = nrows + 3;   // padded columns: the words between n and col_stride do not exist for the last column
    // 16-byte aligned storage for the 16-byte loads; exactly the words the layout owns
    const size_t words = LAYOUT == ROWS_COLUMN_MAJOR ? (size_t)(width - 1) * col_stride + nrows : (size_t)nrows * width;
    // a row-major matrix that takes word loads although its width is a multiple of 4: hand it over 4 bytes off alignment
    const size_t off = (LAYOUT == ROWS_ROW_MAJOR && !vec && width % 4 == 0) ? 1 : 0;
    uint32_t* store = static_cast<uint32_t*>(::operator new((words + off) * sizeof(uint32_t), std::align_val_t(16)));
    uint32_t* m = store + off;
    for (uint32_t i = 0; i < nrows; ++i)
        for (uint32_t c = 0; c < width; ++c)
            m[LAYOUT == ROWS_COLUMN_MAJOR ? c * col_stride + i : (uint64_t)i * width + c] = rows[(size_t)i * width + c];
    for (uint32_t i = 0; i < nrows; ++i) {
        uint32_t sw[4] = {0, 0, 0, 0};
        if (SALTED)
            for (int j = 0; j < 4; ++j)
                sw[j] = (uint32_t)salts[16 * i + 4 * j] | ((uint32_t)salts[16 * i + 4 * j + 1] << 8) | ((uint32_t)salts[16 * i + 4 * j + 2] << 16) |
                        ((uint32_t)salts[16 * i + 4 * j + 3] << 24);
        const Digest d = merkle_row_leaf_at<LAYOUT, SALTED>(m, i, width, col_stride, vec, sw);
        const unsigned msg = 1u + (SALTED ? 16u : 0u) + 8u * width;
        std::printf("%u %d %d %d %u ", width, SALTED ? 1 : 0, LAYOUT, vec ? 1 : 0, (msg + 9u + 63u) / 64u);
        if (SALTED) hex(&salts[16 * i], 16);
        for (uint32_t c = 0; c < width; ++c) {
            const uint64_t v = rows[(size_t)i * width + c];
            uint8_t le[8];
            for (int b = 0; b < 8; ++b) le[b] = (uint8_t)(v >> (8 * b));
            hex(le, 8);
        }
        std::printf(" ");
        uint8_t out[32];
        for (int j = 0; j < 8; ++j)
            for (int b = 0; b < 4; ++b) out[4 * j + b] = (uint8_t)(d.m[j] >> (8 * b));
        hex(out, 32);
        std::printf("\n");
    }
    ::operator delete(store, std::align_val_t(16));
}

int main(int argc, char** argv) {
    const uint32_t max_width = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 40u;
    const uint32_t ROWS = 5;
    for (uint32_t width = 1; width <= max_width; ++width) {
        std::vector<uint32_t> rows((size_t)ROWS * width);
        for (uint32_t i = 0; i < ROWS; ++i)
            for (uint32_t c = 0; c < width; ++c) rows[(size_t)i * width + c] = draw_value(i, c);
        std::vector<uint8_t> salts(16 * ROWS);
        for (auto& b : salts) b = (uint8_t)splitmix();
        run<ROWS_COLUMN_MAJOR, true>(width, false, rows, ROWS, salts);
        run<ROWS_COLUMN_MAJOR, false>(width, false, rows, ROWS, salts);
        run<ROWS_ROW_MAJOR, true>(width, false, rows, ROWS, salts);
        run<ROWS_ROW_MAJOR, false>(width, false, rows, ROWS, salts);
        if (width % 4 == 0) {
            run<ROWS_ROW_MAJOR, true>(width, true, rows, ROWS, salts);
            run<ROWS_ROW_MAJOR, false>(width, true, rows, ROWS, salts);
        }
    }
    std::printf("DONE\n");
    return 0;
}
