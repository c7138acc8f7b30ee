// CPU-only check of the owning buffers and handles every device and pinned allocation of the library goes through
// (csrc/device_alloc.hpp), built with -fsanitize=address,undefined by tests/test_sanitizers.py and run with the leak detector on.
// The header's ownership logic needs nothing of HIP: this program supplies the two raw functions itself (malloc-backed, with a call
// log and a "fail the N-th allocation" switch) and stubs for a stream and an event.  Checked: move construction / assignment, the
// tally and the process-wide counters against the bytes really held, ensure (nothing within capacity; beyond it free BEFORE
// allocate; a failed allocation leaves the buffer empty with capacity 0), constructors that throw after the j-th allocation, and
// maps of move-only structs of buffers (the shape of the sessions' injection and gauge plans).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <new>
#include <string>
#include <utility>
#include <vector>

#define SEPFWI_ALLOC_EXTERNAL
#include "../../sep-2023_amd/csrc/device_alloc.hpp"

using namespace sepfwi;

// ---- the stub behind the seam -------------------------------------------------------------------------------------------------
struct Block {
    Mem kind;
    size_t bytes;
};
static std::map<void *, Block> g_held;  // what is allocated right now
static std::string g_log;               // 'A' per allocation, 'F' per free, in call order
static int g_fail_at = -1, g_allocs = 0;  // fail the g_fail_at-th allocation from now (0-based), -1: none

void *sepfwi::raw_alloc(Mem kind, size_t bytes) {
    if (bytes == 0) std::abort();  // the owners never ask for nothing
    if (g_allocs++ == g_fail_at) throw std::bad_alloc();
    void *p = std::malloc(bytes);
    if (!p) throw std::bad_alloc();
    g_held[p] = Block{kind, bytes};
    g_log += 'A';
    return p;
}

void sepfwi::raw_free(Mem kind, void *p) noexcept {
    auto it = g_held.find(p);
    if (it == g_held.end() || it->second.kind != kind) std::abort();  // a free of what was never given, or through the wrong call
    g_held.erase(it);
    g_log += 'F';
    std::free(p);
}

static long long held(Mem kind) {
    long long s = 0;
    for (auto &kv : g_held)
        if (kv.second.kind == kind) s += (long long)kv.second.bytes;
    return s;
}

static void fail_after(int n) {
    g_fail_at = n;
    g_allocs = 0;
}

static int g_streams = 0, g_events = 0;  // stub handles alive
static void stub_destroy_stream(int *s) {
    g_streams--;
    delete s;
}
static void stub_destroy_event(long *e) {
    g_events--;
    delete e;
}
using StubStream = Handle<int *, stub_destroy_stream>;
using StubEvent = Handle<long *, stub_destroy_event>;
static StubStream stub_stream() {
    g_streams++;
    return StubStream(new int(7));
}
static StubEvent stub_event() {
    g_events++;
    return StubEvent(new long(9));
}

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

// the counters say what the stub holds, and the tally says what its buffers hold
static bool consistent(long long tally, long long want_tally) {
    return tally == want_tally && live_bytes().device.load() == held(Mem::Device) && live_bytes().pinned.load() == held(Mem::Pinned);
}

static int check_move_and_tally() {
    long long tally = 0, ptally = 0;
    {
        DevBuf<float> a(&tally, 10);
        CHECK(a && a.size() == 10 && consistent(tally, 40));
        float *pa = a.get();
        DevBuf<float> b(std::move(a));  // move construction: the block changes hands, nothing is allocated or freed
        CHECK(!a && a.get() == nullptr && a.size() == 0 && b.get() == pa && b.size() == 10 && consistent(tally, 40));
        DevBuf<float> c(&tally, 3);
        CHECK(consistent(tally, 52));
        c = std::move(b);  // move assignment: the target's own block goes, the source is left empty
        CHECK(!b && b.size() == 0 && c.get() == pa && c.size() == 10 && consistent(tally, 40));
        c = std::move(c);  // (self-assignment keeps the block)
        CHECK(c.get() == pa && consistent(tally, 40));
        DevBuf<float> d;  // no tally: counted process-wide only
        d = std::move(c);
        CHECK(d.get() == pa && consistent(tally, 40));  // ... and a moved block stays booked where it was
        PinBuf<int> h(&ptally, 5);
        CHECK(ptally == 20 && consistent(tally, 40) && held(Mem::Pinned) == 20);
        h.reset();
        CHECK(!h && ptally == 0 && held(Mem::Pinned) == 0);
        h.reset();  // (twice is once)
        std::vector<DevBuf<char>> list;  // the shape of the sessions' list of constructor-time blocks
        for (int k = 1; k <= 20; k++) list.push_back(DevBuf<char>(&tally, (size_t)k));
        CHECK(consistent(tally, 40 + 210));
        a.ensure(0);  // nothing asked, nothing done
        CHECK(!a && consistent(tally, 250));
    }
    CHECK(consistent(tally, 0) && ptally == 0 && g_held.empty());
    return 0;
}

static int check_ensure() {
    long long tally = 0;
    DevBuf<double> b(&tally);
    CHECK(!b && b.size() == 0);
    b.ensure(8);
    double *p = b.get();
    g_log.clear();
    b.ensure(8);
    b.ensure(3);
    b.ensure(0);
    CHECK(b.get() == p && b.size() == 8 && g_log.empty() && consistent(tally, 64));  // within capacity: nothing happens
    b.ensure(9);
    CHECK(g_log == "FA" && b.size() == 9 && consistent(tally, 72));  // beyond it: the old block goes BEFORE the new one comes
    // the allocation fails: the exception leaves, the buffer is empty with capacity 0, the tally is back by the old size ...
    fail_after(0);
    g_log.clear();
    bool thrown = false;
    try {
        b.ensure(100);
    } catch (const std::bad_alloc &) {
        thrown = true;
    }
    fail_after(-1);
    CHECK(thrown && g_log == "F" && !b && b.get() == nullptr && b.size() == 0 && consistent(tally, 0) && g_held.empty());
    // ... so that asking for the OLD size again allocates again: no capacity can outlive its block
    g_log.clear();
    b.ensure(9);
    CHECK(g_log == "A" && b && b.size() == 9 && consistent(tally, 72));
    b.reset();
    CHECK(consistent(tally, 0));
    return 0;
}

// k buffers, a stream and an event, as a session holds them: the handles first, so that they go after the buffers
struct Aggregate {
    static constexpr int k = 5;
    StubStream stream;
    StubEvent event;
    PinBuf<float> h_io;
    DevBuf<float> grown;
    std::vector<DevBuf<char>> list;
    DevBuf<int> lane[2];
    explicit Aggregate(long long *tally) : grown(tally) {
        stream = stub_stream();
        event = stub_event();
        list.push_back(DevBuf<char>(tally, 100));  // allocation 0
        list.push_back(DevBuf<char>(tally, 50));   // 1
        grown.ensure(7);                           // 2
        lane[1] = DevBuf<int>(tally, 11);          // 3
        h_io.ensure(13);                           // 4 (pinned: no tally)
    }
};

static int check_throwing_constructors() {
    for (int j = 0; j <= Aggregate::k; j++) {
        long long tally = 0;
        bool thrown = false;
        fail_after(j);  // j == k: the constructor completes
        try {
            Aggregate a(&tally);
            CHECK(j == Aggregate::k && consistent(tally, 100 + 50 + 28 + 44) && held(Mem::Pinned) == 52 && g_streams == 1 && g_events == 1);
        } catch (const std::bad_alloc &) {
            thrown = true;
        }
        fail_after(-1);
        CHECK(thrown == (j < Aggregate::k));
        // nothing is left: not in the tally, the stub or the counters, no handle (and the leak detector sees the rest)
        CHECK(tally == 0 && g_held.empty() && live_bytes().device.load() == 0 && live_bytes().pinned.load() == 0 && g_streams == 0 && g_events == 0);
    }
    return 0;
}

struct Plan {  // move-only by its members, like Session::InjDev / GaugeDev
    DevBuf<int> lookup, start;
    DevBuf<float> w;
    std::vector<int> host;
    int n = 0;
};

static int check_maps() {
    long long tally = 0;
    {
        std::map<int, Plan> plans;
        for (int id : {7, 3, 11}) {
            Plan p;
            p.lookup = DevBuf<int>(&tally, (size_t)id);
            p.start = DevBuf<int>(&tally, 2);
            p.w = DevBuf<float>(&tally, (size_t)(2 * id));
            p.host.assign((size_t)id, id);
            p.n = id;
            const int *lk = p.lookup.get();
            Plan &q = plans.emplace(id, std::move(p)).first->second;
            CHECK(q.lookup.get() == lk && q.n == id && !p.lookup && !p.w);
        }
        CHECK(consistent(tally, (7 + 3 + 11) * 12 + 3 * 8));
        const Plan *before = &plans.find(3)->second;
        Plan extra;
        extra.lookup = DevBuf<int>(&tally, 1);
        CHECK(!plans.emplace(3, std::move(extra)).second && &plans.find(3)->second == before);  // (nodes are stable; a refused emplace frees its own)
        CHECK(plans.find(11)->second.w.size() == 22 && plans.find(5) == plans.end());
        plans.erase(7);
        CHECK(consistent(tally, (3 + 11) * 12 + 2 * 8 + (extra.lookup ? 4 : 0)));
    }
    CHECK(consistent(tally, 0) && g_held.empty());
    return 0;
}

int main() {
    if (check_move_and_tally() || check_ensure() || check_throwing_constructors() || check_maps()) return 1;
    if (!g_held.empty() || live_bytes().device.load() != 0 || live_bytes().pinned.load() != 0) {
        std::printf("FAILED: blocks left at exit\n");
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
