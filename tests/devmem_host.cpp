// Stand-alone driver of fwi::DeviceMemory (csrc/fwi_devmem.h) on the CPU: a fake allocator over malloc that counts its
// live blocks, can fail the n-th allocation, can refuse the free of one base, and aborts on a double or unknown free.
// Built with -fsanitize=address,undefined and run by tests/test_devmem_host.py; exit status 0 = every case held.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>

#include "fwi_devmem.h"

using fwi::DeviceMemory;

namespace {

struct Fake {
    std::set<void *> live;
    int allocs = 0, frees = 0;
    int fail_at = -1;          // the allocation (counted from 0 over the fake's life) that fails with code 2
    void *refuse[2] = {};      // bases whose free is refused with code 17: the block stays live in the fake
    char *arena = nullptr;     // when set: blocks are carved from it back to back (adjacent ranges), not from malloc
    size_t arena_used = 0;
} fake;

int fake_alloc(void **p, size_t bytes) {
    if (fake.allocs++ == fake.fail_at) return 2;
    if (fake.arena) {
        *p = fake.arena + fake.arena_used;
        fake.arena_used += bytes;
    } else {
        *p = malloc(bytes);
    }
    fake.live.insert(*p);
    return 0;
}

int fake_free(void *p) {
    if (!fake.live.count(p)) {
        fprintf(stderr, "fake_free: %p is not a live base (double or unknown free)\n", p);
        abort();
    }
    if (p == fake.refuse[0] || p == fake.refuse[1]) return 17;
    fake.live.erase(p);
    ++fake.frees;
    if (!fake.arena) free(p);
    return 0;
}

int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

void round_trip() {
    DeviceMemory mem(fake_alloc, fake_free);
    void *a = nullptr;
    CHECK(mem.acquire(&a, 100, "a") == 0 && a);
    CHECK(mem.blocks() == 1 && mem.bytes() == 100 && fake.live.size() == 1);
    CHECK(mem.release(&a) == 0 && a == nullptr);
    CHECK(mem.blocks() == 0 && mem.bytes() == 0 && fake.live.empty());
}

void interior_pointers() {
    DeviceMemory mem(fake_alloc, fake_free);
    for (size_t off : {(size_t)1, (size_t)63}) {  // moved 1 byte into the block; at bytes - 1
        void *a = nullptr;
        CHECK(mem.acquire(&a, 64, "a") == 0);
        a = (char *)a + off;
        CHECK(mem.release(&a) == 0 && a == nullptr && mem.blocks() == 0 && fake.live.empty());
    }
    // one past the end of the first of two blocks: the second one's where that is its base, else nobody's; never the first
    static char arena[128];
    for (bool adjacent : {false, true}) {
        fake.arena = adjacent ? arena : nullptr;
        fake.arena_used = 0;
        void *a = nullptr, *b = nullptr;
        CHECK(mem.acquire(&a, 64, "a") == 0 && mem.acquire(&b, 64, "b") == 0);
        void *end = (char *)a + 64;
        const bool second = end == b;
        CHECK(!adjacent || second);
        const int rc = mem.release(&end);
        if (second) {
            CHECK(rc == 0 && end == nullptr && !fake.live.count(b));
            b = nullptr;
        } else {
            CHECK(rc == DeviceMemory::UNKNOWN && end == (char *)a + 64);
        }
        CHECK(fake.live.count(a) == 1 && mem.blocks() == (second ? 1u : 2u));
        CHECK(mem.release(&a) == 0 && mem.release(&b) == 0 && mem.blocks() == 0 && fake.live.empty());
        fake.arena = nullptr;
    }
}

void null_and_foreign() {
    DeviceMemory mem(fake_alloc, fake_free);
    void *a = nullptr, *none = nullptr;
    CHECK(mem.acquire(&a, 32, "a") == 0);
    const int frees = fake.frees;
    CHECK(mem.release(&none) == 0 && none == nullptr);
    char elsewhere[8];
    void *foreign = elsewhere;
    CHECK(mem.release(&foreign) == DeviceMemory::UNKNOWN && DeviceMemory::UNKNOWN != 0);
    CHECK(foreign == (void *)elsewhere && fake.frees == frees && mem.blocks() == 1 && mem.bytes() == 32);
    CHECK(mem.release(&a) == 0 && fake.live.empty());
}

void failed_acquire() {
    DeviceMemory mem(fake_alloc, fake_free);
    void *s[3] = {};
    fake.fail_at = fake.allocs + 1;
    CHECK(mem.acquire(&s[0], 10, "s", 0) == 0);
    s[1] = &mem;  // (whatever the slot held: it reads null after the failure)
    CHECK(mem.acquire(&s[1], 20, "s", 1) == 2 && s[1] == nullptr);
    CHECK(mem.blocks() == 1 && mem.bytes() == 10);
    CHECK(mem.acquire(&s[2], 30, "s", 2) == 0);
    CHECK(mem.blocks() == 2 && mem.bytes() == 40 && fake.live.size() == 2);
    fake.fail_at = -1;
    int reports = 0;
    mem.release_all([&](const char *, int, int) { ++reports; });
    CHECK(reports == 0 && mem.blocks() == 0 && fake.live.empty());
}

void release_all_cases() {
    {  // every base once, also when two slots changed roles (adopt) and one was moved (tune_placement)
        DeviceMemory mem(fake_alloc, fake_free);
        void *u = nullptr, *fx = nullptr, *ty = nullptr;
        CHECK(mem.acquire(&u, 48, "u") == 0 && mem.acquire(&fx, 48, "fx") == 0 && mem.acquire(&ty, 96, "pml_ty") == 0);
        std::swap(u, fx);
        ty = (char *)ty + 32;
        const int frees = fake.frees;
        mem.release_all([](const char *, int, int) { CHECK(false && "no free was refused"); });
        CHECK(fake.frees == frees + 3 && fake.live.empty() && mem.blocks() == 0 && mem.bytes() == 0);
        mem.release_all([](const char *, int, int) { CHECK(false && "nothing is held"); });  // (a double free would abort)
    }
    {  // refused frees: the rest is freed, the first refusal alone is reported, with the block's member and index
        DeviceMemory mem(fake_alloc, fake_free);
        void *s[5] = {};
        for (int i = 0; i < 5; ++i) CHECK(mem.acquire(&s[i], 16, i < 3 ? "vecs" : "pml_a", i % 3) == 0);
        fake.refuse[0] = s[1];
        fake.refuse[1] = s[3];
        int reports = 0;
        std::string member;
        int index = -1, code = 0;
        mem.release_all([&](const char *m, int i, int rc) {
            ++reports;
            member = m;
            index = i;
            code = rc;
        });
        CHECK(reports == 1 && member == "vecs" && index == 1 && code == 17);
        CHECK(mem.blocks() == 0 && fake.live.size() == 2 && fake.live.count(s[1]) && fake.live.count(s[3]));
        fake.refuse[0] = fake.refuse[1] = nullptr;  // (the fake's own clean-up, for the leak check)
        CHECK(fake_free(s[1]) == 0 && fake_free(s[3]) == 0);
    }
    {  // release(): a refused free still leaves a null slot and no record
        DeviceMemory mem(fake_alloc, fake_free);
        void *a = nullptr;
        CHECK(mem.acquire(&a, 16, "a") == 0);
        void *base = fake.refuse[0] = a;
        CHECK(mem.release(&a) == 17 && a == nullptr && mem.blocks() == 0);
        fake.refuse[0] = nullptr;
        CHECK(fake_free(base) == 0);
    }
}

void growth() {  // as ensure() grows a buffer: release, then acquire larger on the same slot
    DeviceMemory mem(fake_alloc, fake_free);
    void *b = nullptr;
    CHECK(mem.acquire(&b, 16, "data_tmp") == 0);
    void *old = b;
    CHECK(mem.release(&b) == 0 && !fake.live.count(old));
    CHECK(mem.acquire(&b, 4096, "data_tmp") == 0 && b);
    CHECK(mem.blocks() == 1 && mem.bytes() == 4096 && fake.live.size() == 1);
    mem.release_all([](const char *, int, int) { CHECK(false && "no free was refused"); });
    CHECK(fake.live.empty());
}

}  // namespace

int main() {
    round_trip();
    interior_pointers();
    null_and_foreign();
    failed_acquire();
    release_all_cases();
    growth();
    CHECK(fake.live.empty() && fake.allocs - 1 == fake.frees);  // (one allocation was made to fail)
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
