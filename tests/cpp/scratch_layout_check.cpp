// scratch_layout_check.cpp — host-only check of csrc/scratch_layout.hpp (tests/test_scratch_layout.py compiles and runs it).
// Prints "ok <number of layouts checked>" and returns 0, or the first violated property and 1.  With the argument "overflow" it declares
// one slot more than the capacity, which must abort: it prints "full" before that slot and "survived" (exit 2) if add() returns.
#include "scratch_layout.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>

using pcr::Layout;

namespace {

struct alignas(16) Vec16 { unsigned char b[16]; };

const size_t COUNTS[] = { 0, 1, 63, 64, 65, 2049 };
constexpr int N_COUNTS = sizeof COUNTS / sizeof COUNTS[0];
const unsigned char GUARD = 0xA5;

int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (!fails) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } fails++; } } while (0)

// the pointers a layout binds, between two guard words that bind() must leave alone
struct Targets {
    unsigned char before[64];
    void* p[Layout::CAP + 1];
    unsigned char after[64];
};

template <class T> void add_one(Layout& L, void** p, size_t count) { L.add((T**)p, count); }

void add_slot(Layout& L, void** p, int elem, size_t count)
{
    switch (elem) {
    case 1: add_one<uint8_t>(L, p, count); break;
    case 4: add_one<uint32_t>(L, p, count); break;
    case 8: add_one<double>(L, p, count); break;
    case 16: add_one<Vec16>(L, p, count); break;
    default: L.add(p, count); break;             // 0: the raw byte slot
    }
}

// one layout of n_slots slots; slot i holds COUNTS[(i + shift) % N_COUNTS] elements of ELEMS[(i + shift2) % 5] bytes
int check_layout(int n_slots, int shift, int shift2)
{
    static const int ELEMS[] = { 1, 4, 8, 16, 0 };
    Targets t;
    std::memset(&t, GUARD, sizeof t);
    Layout L;
    size_t want[Layout::CAP];
    for (int i = 0; i < n_slots; i++) {
        const int elem = ELEMS[(i + shift2) % 5];
        const size_t count = COUNTS[(i + shift) % N_COUNTS];
        want[i] = count * (size_t)(elem ? elem : 1);
        add_slot(L, &t.p[i], elem, count);
    }
    alignas(256) static unsigned char arena[1];   // only its address is used
    unsigned char* base = arena;
    L.bind(base);
    size_t end = 0;
    for (int i = 0; i < n_slots; i++) {
        const size_t off = (size_t)((unsigned char*)t.p[i] - base);
        CHECK(off % 256 == 0, "slot %d of %d at offset %zu", i, n_slots, off);
        CHECK(off >= end, "slot %d of %d at %zu overlaps the previous slot's end %zu", i, n_slots, off, end);
        CHECK(off <= L.bytes(), "slot %d of %d at %zu lies outside the %zu bytes", i, n_slots, off, L.bytes());
        end = off + want[i];
    }
    CHECK(L.bytes() >= end, "bytes() = %zu < end of the last slot %zu", L.bytes(), end);
    CHECK(L.bytes() % 256 == 0, "bytes() = %zu", L.bytes());
    for (size_t k = 0; k < sizeof t.before; k++) CHECK(t.before[k] == GUARD && t.after[k] == GUARD, "bind wrote outside the registered pointers");
    for (int i = n_slots; i <= Layout::CAP; i++) {
        void* g;
        std::memset(&g, GUARD, sizeof g);
        CHECK(t.p[i] == g, "bind wrote pointer %d of a layout of %d slots", i, n_slots);
    }
    return 1;
}

// one slot past the capacity is a hard error: add() aborts, and nothing was written through the refused pointer before that
int run_overflow()
{
    static void* p[Layout::CAP + 1];
    Layout L;
    for (int i = 0; i < Layout::CAP; i++) L.add((uint32_t**)&p[i], 7);
    L.bind(nullptr);
    std::printf("full %zu\n", L.bytes());
    std::fflush(stdout);
    L.add((uint32_t**)&p[Layout::CAP], 7);
    std::printf("survived\n");
    return 2;
}

// The persistent block of the matrix-core index (bt_ensure, grid.hip): the search kernels read it on the hot path, so the offsets the
// Layout gives must equal the expression the block was carved with before, written out here as plain arithmetic.
void check_bt_block(size_t n)
{
    const size_t BT_SUPER = 256, GR_BLOCK = 256, F4 = 16, U4 = 16;
    const size_t n_super = (n + BT_SUPER - 1) / BT_SUPER, n_pad = n_super * BT_SUPER, n_tiles = n_pad / 32;
    const size_t bb_blocks = std::min<size_t>(256, (n + GR_BLOCK - 1) / GR_BLOCK);
    const size_t off_cen = n_pad * F4, off_ops = off_cen + ((n_super * F4 + 255) & ~(size_t)255),
                 off_o16 = off_ops + n_tiles * 128 * U4, off_bb = off_o16 + n_tiles * 64 * U4,
                 off_flag = off_bb + ((bb_blocks * 6 * sizeof(float) + 255) & ~(size_t)255), total = off_flag + 256;
    Vec16 *records, *centres, *ops, *ops16;
    float* bb;
    int* bad16;
    Layout L;
    L.add(&records, n_pad);
    L.add(&centres, n_super);
    L.add(&ops, n_tiles * 128);
    L.add(&ops16, n_tiles * 64);
    L.add(&bb, bb_blocks * 6);
    L.add(&bad16, 1);
    L.bind(nullptr);
    const size_t got[6] = { (size_t)records, (size_t)centres, (size_t)ops, (size_t)ops16, (size_t)bb, (size_t)bad16 };
    const size_t want[6] = { 0, off_cen, off_ops, off_o16, off_bb, off_flag };
    for (int i = 0; i < 6; i++) CHECK(got[i] == want[i], "bt block, n = %zu: slot %d at %zu, was %zu", n, i, got[i], want[i]);
    CHECK(L.bytes() == total, "bt block, n = %zu: %zu bytes, was %zu", n, L.bytes(), total);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "overflow") == 0) return run_overflow();
    int layouts = 0;
    for (int n_slots = 0; n_slots <= Layout::CAP; n_slots++)
        for (int shift = 0; shift < N_COUNTS; shift++)
            for (int shift2 = 0; shift2 < 5; shift2++) layouts += check_layout(n_slots, shift, shift2);
    {   // an empty layout is legal: no bytes, bind succeeds and writes nothing (checked above with n_slots = 0)
        Layout L;
        CHECK(L.bytes() == 0, "empty layout has %zu bytes", L.bytes());
        L.bind(nullptr);
    }
    for (size_t n : { (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)120000 }) check_bt_block(n);
    CHECK(pcr::al256(0) == 0 && pcr::al256(1) == 256 && pcr::al256(256) == 256 && pcr::al256(257) == 512, "al256");
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok %d\n", layouts);
    return 0;
}
