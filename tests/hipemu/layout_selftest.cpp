// BlockLayout (robo_amd/csrc/block_layout.h) against its rule, restated here: every array starts at the running sum of the
// sizes before it, each rounded up to the alignment; a count of 0 takes nothing.  A stand-alone program on the header alone:
// exit status 0 and "layout selftest ok", or 1 and the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../robo_amd/csrc/block_layout.h"

using robo::BlockLayout;

struct Rec20 {
    char bytes[20];
};
static_assert(sizeof(Rec20) == 20, "the odd-sized element of the sequences");

enum Type { F64, I64, I32, U32, R20, CF64, CR20 };     // C..: through the const overload
struct Item {
    Type type;
    size_t count;
};

static const std::vector<std::vector<Item>> SEQUENCES = {
    {{F64, 3}, {I64, 1}, {I32, 5}, {U32, 1}, {R20, 3}, {F64, 7}},
    {{I32, 1}, {F64, 0}, {I32, 3}, {R20, 1}, {I64, 0}, {U32, 7}, {F64, 1}},
    {{R20, 5}, {CF64, 9}, {I32, 0}, {I32, 0}, {CR20, 2}, {U32, 3}, {I64, 11}},
    {{U32, 0}, {F64, 1}},
    {{CF64, 13}, {I32, 1}, {I64, 3}, {F64, 0}},        // ends on an empty array: bound to the end of the block
    {},
};

static size_t size_of(Type t) {
    switch (t) {
        case F64: case CF64: return sizeof(double);
        case I64: return sizeof(long long);
        case I32: return sizeof(int);
        case U32: return sizeof(unsigned);
        default: return sizeof(Rec20);
    }
}

[[noreturn]] static void fail(size_t align, size_t seq, size_t item, const char* what, size_t got, size_t want) {
    fprintf(stderr, "layout selftest: align %zu, sequence %zu, entry %zu: %s is %zu, expected %zu\n", align, seq, item, what, got,
            want);
    exit(1);
}

// one pointer of every type per entry; an entry uses the one of its type
struct Field {
    double* f64;
    long long* i64;
    int* i32;
    unsigned* u32;
    Rec20* r20;
    const double* cf64;
    const Rec20* cr20;
    const void* bound(Type t) const {
        switch (t) {
            case F64: return f64;
            case I64: return i64;
            case I32: return i32;
            case U32: return u32;
            case R20: return r20;
            case CF64: return cf64;
            default: return cr20;
        }
    }
};

static void check(size_t align, size_t si) {
    const std::vector<Item>& seq = SEQUENCES[si];
    std::vector<Field> fields(seq.size(), Field{});
    std::vector<size_t> want(seq.size());
    BlockLayout lay(align);
    size_t sum = 0;
    for (size_t i = 0; i < seq.size(); ++i) {
        const size_t n = seq[i].count;
        Field& f = fields[i];
        size_t got = 0;
        switch (seq[i].type) {
            case F64: got = lay.add(&f.f64, n); break;
            case I64: got = lay.add(&f.i64, n); break;
            case I32: got = lay.add(&f.i32, n); break;
            case U32: got = lay.add(&f.u32, n); break;
            case R20: got = lay.add(&f.r20, n); break;
            case CF64: got = lay.add(&f.cf64, n); break;
            case CR20: got = lay.add(&f.cr20, n); break;
        }
        want[i] = sum;
        if (got != sum) fail(align, si, i, "the offset", got, sum);
        const size_t before = sum;
        sum += (n * size_of(seq[i].type) + align - 1) / align * align;
        if (n == 0 && lay.bytes() != before) fail(align, si, i, "bytes() behind an empty array", lay.bytes(), before);
        if (lay.bytes() != sum) fail(align, si, i, "bytes()", lay.bytes(), sum);
    }
    if (lay.bytes() != sum) fail(align, si, seq.size(), "the total", lay.bytes(), sum);
    // bind against a real allocation (one spare byte: an empty block or an empty last array points at its end)
    std::vector<char> block(sum + 1);
    lay.bind(block.data());
    for (size_t i = 0; i < seq.size(); ++i) {
        const char* p = static_cast<const char*>(fields[i].bound(seq[i].type));
        if (p != block.data() + want[i])
            fail(align, si, i, "the bound address (as an offset)", (size_t)(p - block.data()), want[i]);
    }
}

int main() {
    for (size_t align : {(size_t)8, (size_t)16})
        for (size_t si = 0; si < SEQUENCES.size(); ++si) check(align, si);
    printf("layout selftest ok: %zu sequences x 2 alignments\n", SEQUENCES.size());
    return 0;
}
