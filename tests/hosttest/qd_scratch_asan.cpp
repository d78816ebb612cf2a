// qd_scratch_asan.cpp -- the sequences of tests/test_scratch_cpu.py once more, on a malloc-backed memory policy in a program
// of its own that is built with -fsanitize=address,undefined: a leak, a double free, a use after free or a block shorter
// than its capacity is reported by the sanitizer and ends the program with a non-zero status.  TEST INFRASTRUCTURE.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "qd_scratch.h"

struct Heap {
    static int fail_in;                                // > 0: the fail_in-th next allocation fails
    static int alloc(void** p, size_t bytes) {
        if (fail_in > 0 && --fail_in == 0) return 2;
        *p = malloc(bytes);
        return *p ? 0 : 2;
    }
    static int release(void* p) { free(p); return 0; }
};
int Heap::fail_in = 0;
typedef QdBuf<double, Heap> Buf;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "qd_scratch_asan.cpp:%d: %s\n", __LINE__, #c); return 1; } } while (0)

// every double of the block is written and read back: the sanitizer sees the capacity
static bool usable(Buf& b) {
    for (size_t i = 0; i < b.cap; ++i) b.p[i] = (double)i;
    double sum = 0.0;
    for (size_t i = 0; i < b.cap; ++i) sum += b.p[i];
    return sum == 0.5 * (double)b.cap * (double)(b.cap - 1);
}

static int one_buffer() {
    Buf b;
    CHECK(!b.p && b.cap == 0);
    CHECK(b.reserve(100) == 0 && b.p && b.cap >= 100 && usable(b));
    double* first = b.p;
    CHECK(b.reserve(100) == 0 && b.reserve(7) == 0 && b.reserve(0) == 0 && b.p == first && b.cap >= 100);
    CHECK(b.reserve(1000) == 0 && b.cap >= 1000 && usable(b));
    Heap::fail_in = 1;
    CHECK(b.reserve(5000) == 2 && !b.p && b.cap == 0);             // a failed growth: empty
    CHECK(b.reserve(10) == 0 && b.cap >= 10 && usable(b));         // and a smaller reserve succeeds
    b.release();
    CHECK(!b.p && b.cap == 0);
    b.release();                                                    // (releasing an empty buffer does nothing)
    CHECK(b.reserve(3) == 0 && usable(b));
    return 0;                                                       // the destructor frees the last block
}

static int group_of_four() {
    const size_t small[4] = {10, 20, 30, 40}, large[4] = {100, 200, 300, 400};
    for (int start = 0; start < 2; ++start)                         // from an empty group and from an allocated one
        for (int fail = 1; fail <= 4; ++fail) {
            Buf b[4];
            Buf* const g[] = {&b[0], &b[1], &b[2], &b[3]};
            if (start) {
                CHECK(qd_reserve_group(g, small) == 0);
                for (int k = 0; k < 4; ++k) CHECK(b[k].cap >= small[k] && usable(b[k]));
            }
            Heap::fail_in = fail;
            CHECK(qd_reserve_group(g, large) == 2);
            for (int k = 0; k < 4; ++k) CHECK(!b[k].p && b[k].cap == 0);
            CHECK(Heap::fail_in == 0);
            CHECK(qd_reserve_group(g, large) == 0);
            for (int k = 0; k < 4; ++k) CHECK(b[k].cap >= large[k] && usable(b[k]));
        }
    return 0;
}

int main() {
    if (one_buffer() || group_of_four()) return 1;
    printf("qd_scratch_asan ok\n");
    return 0;
}
