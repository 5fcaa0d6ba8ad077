// TEST INFRASTRUCTURE: the owner of device blocks of csrc/hpf_devmem.hpp on the host (tests/test_devmem_host.py), on a backend of malloc / free
// whose k-th allocation can be made to fail with either kind of error: all-or-nothing groups, clear() and the destructor, re-allocation of one
// block, count == 0, uploads, and the live counters after every sequence.  Prints "devmem clean" when every check holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>

#include "hpf_devmem.hpp"
using namespace hpf;

static int fails = 0;
#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c);  \
            ++fails;                                             \
        }                                                        \
    } while (0)

struct FakeBackend {
    static constexpr int oom = 2, other = 709;
    static int fail_at, fail_code, copy_code;             // the fail_at-th allocation from now (1-based; 0: none) fails with fail_code
    static std::set<void*> live;                          // every block handed out and not yet freed
    static int alloc(void** p, size_t bytes) {
        if (fail_at > 0 && --fail_at == 0) return fail_code;
        *p = malloc(bytes);
        live.insert(*p);
        return 0;
    }
    static int free(void* p) {
        CHECK(live.erase(p) == 1);                         // (a block freed twice, or one this backend never gave out)
        ::free(p);
        return 0;
    }
    static int copy_in(void* dst, const void* src, size_t bytes) {
        if (copy_code) return copy_code;
        memcpy(dst, src, bytes);
        return 0;
    }
};
int FakeBackend::fail_at = 0, FakeBackend::fail_code = 0, FakeBackend::copy_code = 0;
std::set<void*> FakeBackend::live;
using Owner = DevOwner<FakeBackend>;

static int64_t live_blocks() { return devmem_live().blocks.load(); }
static int64_t live_bytes() { return devmem_live().bytes.load(); }

// a group of three buffers of different types, all-or-nothing: the pattern of every group of the handle
struct Group {
    double* a = nullptr;
    int* b = nullptr;
    long long* c = nullptr;
    int detail = 0;
    Owner mem{&detail};
    int alloc() {
        int r;
        if ((r = mem.alloc(&a, 100)) || (r = mem.alloc(&b, 7)) || (r = mem.alloc(&c, 3))) {
            mem.clear();
            return r;
        }
        return HPF_OK;
    }
};

int main() {
    const int64_t blocks0 = live_blocks(), bytes0 = live_bytes();
    CHECK(blocks0 == 0 && bytes0 == 0);

    // a group of three, the k-th allocation failing with either kind of error; then the retry
    for (int k = 1; k <= 3; ++k)
        for (int kind = 0; kind < 2; ++kind) {
            Group g;
            const int64_t b0 = live_blocks(), y0 = live_bytes();
            FakeBackend::fail_at = k;
            FakeBackend::fail_code = kind ? FakeBackend::other : FakeBackend::oom;
            const int r = g.alloc();
            CHECK(r == (kind ? HPF_E_HIP : HPF_E_NOMEM));
            CHECK(g.detail == FakeBackend::fail_code);
            CHECK(!g.a && !g.b && !g.c && g.mem.empty());
            CHECK(live_blocks() == b0 && live_bytes() == y0 && FakeBackend::live.empty());
            CHECK(FakeBackend::fail_at == 0);
            CHECK(g.alloc() == HPF_OK);
            CHECK(g.a && g.b && g.c && g.mem.blocks() == 3);
            CHECK(live_blocks() == b0 + 3 && live_bytes() == y0 + (int64_t)(100 * sizeof(double) + 7 * sizeof(int) + 3 * sizeof(long long)));
            g.a[99] = 1.0;                                 // (the blocks have the size asked for: ASan watches)
            g.b[6] = 1;
            g.c[2] = 1;
            g.mem.clear();                                 // clear(): pointers null, counters back
            CHECK(!g.a && !g.b && !g.c && live_blocks() == b0 && live_bytes() == y0);
            CHECK(g.alloc() == HPF_OK);                    // ... and the owner is usable again; this time the destructor releases
        }
    CHECK(live_blocks() == blocks0 && live_bytes() == bytes0 && FakeBackend::live.empty());

    // the destructor nulls the recorded pointer variables (they outlive the owner) and returns the counters
    {
        double* p = nullptr;
        float* q = nullptr;
        {
            Owner o;
            CHECK(o.alloc(&p, 10) == HPF_OK && o.alloc(&q, 10) == HPF_OK && p && q);
            CHECK(live_blocks() == blocks0 + 2);
        }
        CHECK(!p && !q && live_blocks() == blocks0 && live_bytes() == bytes0 && FakeBackend::live.empty());
    }

    // re-allocating one block (a history buffer that grows): the old block is freed, the records hold the variable once
    {
        Owner o;
        double *hist = nullptr, *other = nullptr;
        CHECK(o.alloc(&other, 5) == HPF_OK);
        CHECK(o.alloc(&hist, 8) == HPF_OK);
        for (int cap = 16; cap <= 64; cap *= 2) {
            CHECK(o.alloc(&hist, (size_t)cap) == HPF_OK && hist);
            hist[cap - 1] = 0.0;
            CHECK(o.blocks() == 2 && live_blocks() == blocks0 + 2 && FakeBackend::live.size() == 2);
            CHECK(live_bytes() == bytes0 + (int64_t)((5 + cap) * sizeof(double)));
        }
        FakeBackend::fail_at = 1;                          // a failed growth: the old block is gone, the variable null, nothing stale in the records
        FakeBackend::fail_code = FakeBackend::oom;
        CHECK(o.alloc(&hist, 128) == HPF_E_NOMEM && !hist && o.blocks() == 1 && live_blocks() == blocks0 + 1);
        CHECK(o.alloc(&hist, 128) == HPF_OK && hist && o.blocks() == 2);
        o.release(&other);                                 // releasing one block leaves the others alone
        CHECK(!other && hist && o.blocks() == 1 && live_blocks() == blocks0 + 1);
        o.release(&other);                                 // (not held: nothing happens)
        CHECK(o.blocks() == 1);
    }
    CHECK(live_blocks() == blocks0 && live_bytes() == bytes0 && FakeBackend::live.empty());

    // count == 0: one element; uploads: pointer + count, std::vector, an empty vector, a failed copy
    {
        Owner o;
        int detail = 0;
        Owner od(&detail);
        double* z = nullptr;
        CHECK(o.alloc(&z, 0) == HPF_OK && z && live_bytes() == bytes0 + (int64_t)sizeof(double));
        z[0] = 1.0;
        const std::vector<int> v = {3, 1, 4, 1, 5};
        int *u = nullptr, *w = nullptr, *e = nullptr, *f = nullptr;
        CHECK(o.upload(&u, v) == HPF_OK && u && !memcmp(u, v.data(), sizeof(int) * v.size()));
        CHECK(o.upload(&w, v.data() + 1, 3) == HPF_OK && w[0] == 1 && w[2] == 1);
        CHECK(o.upload(&e, std::vector<int>()) == HPF_OK && e);
        FakeBackend::copy_code = FakeBackend::other;
        CHECK(od.upload(&f, v) == HPF_E_HIP && detail == FakeBackend::other && od.blocks() == 1);    // (the block stays with the owner)
        FakeBackend::copy_code = 0;
        FakeBackend::fail_at = 1;
        FakeBackend::fail_code = FakeBackend::other;
        int* g2 = nullptr;
        CHECK(od.upload(&g2, v) == HPF_E_HIP && !g2 && od.blocks() == 1);
    }
    CHECK(live_blocks() == blocks0 && live_bytes() == bytes0 && FakeBackend::live.empty());

    if (fails == 0) printf("devmem clean\n");
    return fails ? 1 : 0;
}
