// Sanitizer tier: the device-wide scheduler (algoplonk_amd/csrc/device_sched.h) and the gates attached to it (slot_gate.h), hammered
// from 96 threads under -fsanitize=thread (or address).  Built by `make -C algoplonk_amd/csrc SAN=thread san-sched`, run by
// tests/test_device_sched.py in the CPU tier.  What runs here is the library's own code, not a model of it.
//
// Set-up of the main run: three gates on ONE scheduler of 16 streams - A: 16 slots, B: 32 slots in gangs of up to 2, C: 4 slots -
// and a gate D on the scheduler of a second device ordinal.  Every breach of one of these counts as a violation (exit code 1):
//   * streams held never exceed max_streams, no stream id is held by two leads at once
//   * the members of a gang all hold their lead's stream id (checked where they meet, as the prover's merge points do)
//   * the load a context reads includes the other contexts' proofs (a parked, deterministic scene on top of the running checks)
//   * a lead that began to wait for a stream earlier is served no later than one that began after it, across contexts
//   * every thread finishes its quota within the time limit (no lost wake-up): exit code 2 otherwise
//   * the second ordinal never sees the first one's callers
//   * a gate that detaches while the others run leaves their counts consistent, and the scheduler ends at zero
//   * 16 + 16 callers on two ganging contexts form gangs (each context alone has no more callers than streams); 8 + 8 form none
// The sanitizer reports races on its own and fails the run through TSAN_OPTIONS=halt_on_error=1.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include <unistd.h>

#include "../../algoplonk_amd/csrc/device_sched.h"
#include "../../algoplonk_amd/csrc/slot_gate.h"
#include "../../algoplonk_amd/csrc/gang.h"

using namespace apk;

static constexpr int MAX_STREAMS = 16;
static constexpr int TIME_LIMIT_S = 300;

// join with a limit: a lost wake-up leaves a thread asleep for ever, and the run must say so instead of hanging
static bool join_all(std::vector<std::thread>& th, std::atomic<int>& finished, const char* what) {
    const auto t0 = std::chrono::steady_clock::now();
    while (finished.load() < (int)th.size()) {
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(TIME_LIMIT_S)) {
            printf("%s: %d of %zu threads finished within %d s - a lost wake-up\n", what, finished.load(), th.size(), TIME_LIMIT_S);
            fflush(stdout);
            _exit(2);
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(5));
    }
    for (auto& t : th) t.join();
    return true;
}

// every thread of a scene starts its rounds together, however slowly a busy machine spawns them: the scenes are about crowding
static void start_together(std::atomic<int>& ready, int total) {
    ready++;
    while (ready.load() < total) std::this_thread::sleep_for(std::chrono::microseconds(100));
}

struct Ctx {     // a context as the hammer sees it: its gate, a gang per slot, who holds which slot
    std::unique_ptr<SlotGate> gate{new SlotGate()};
    std::vector<Gang> gangs;
    std::vector<std::atomic<int>> owner;
    int slots, gang_max, dev;
    std::atomic<int> ganged{0}, proofs{0};
    Ctx(int slots_, int gang_max_, int dev_) : gangs((size_t)slots_), owner((size_t)slots_), slots(slots_), gang_max(gang_max_), dev(dev_) {
        for (auto& o : owner) o = 0;
    }
};

struct Dev {
    std::unique_ptr<DeviceSched> sched{new DeviceSched(MAX_STREAMS, true)};
    std::vector<std::atomic<int>> stream_owner;
    std::atomic<int> held{0};
    std::mutex mu;
    std::vector<std::pair<uint64_t, uint64_t>> order;     // (waited, served) of every lead that had to wait for a stream
    Dev() : stream_owner((size_t)MAX_STREAMS) { for (auto& o : stream_owner) o = 0; }
};

// one "proof": through the gate, the checks, a gang's meetings or a lone caller's while, and out again
static void one_proof(Ctx& c, Dev& d, bool allow_gang, std::atomic<int>& bad, int hold_us) {
    SlotGate& gate = *c.gate;
    const SlotGate::Ticket tk = gate.acquire_member(allow_gang);
    if (c.owner[tk.slot].fetch_add(1) != 0) bad++;                                       // two owners of one slot
    if (tk.stream < 0 || tk.stream >= MAX_STREAMS) bad++;
    const bool leads = tk.lead == tk.slot;
    if (leads) {
        if (d.stream_owner[(size_t)tk.stream].fetch_add(1) != 0) bad++;                  // one stream id, two leads
        if (d.held.fetch_add(1) + 1 > MAX_STREAMS) bad++;                                // more streams held than the device has
        if (tk.waited) { std::lock_guard<std::mutex> lk(d.mu); d.order.emplace_back(tk.waited, tk.served); }
    } else if (tk.waited || tk.served) bad++;
    if (tk.size < 1 || tk.size > c.gang_max || tk.idx < 0 || tk.idx >= tk.size || (tk.size == 1 && !leads)) bad++;
    {
        int own = 0;
        const int load = gate.load(&own);
        if (own < 1 || own > c.slots || load < own) bad++;         // the device's figure holds this context's
        const DeviceSched::Counts k = d.sched->read(false);
        if (k.streams_in_use > (uint32_t)MAX_STREAMS || k.streams_peak > (uint32_t)MAX_STREAMS || k.max_streams != (uint32_t)MAX_STREAMS) bad++;
        if (k.proofs_in_flight < 1) bad++;
    }
    c.proofs++;
    if (tk.size > 1) {
        c.ganged++;
        Gang& g = c.gangs[tk.lead];
        g.enter(tk.gen, tk.size);
        struct Args { int stream; int first; };
        const Gang::Launcher launcher = [](GangReq* const* reqs, int count) {
            const int s0 = static_cast<Args*>(reqs[0]->args)->stream;
            for (int i = 0; i < count; i++) { static_cast<Args*>(reqs[i]->args)->first = s0; reqs[i]->rc = count; }
        };
        for (int m = 0; m < 3; m++) {
            Args a{tk.stream, -1};
            GangReq q;
            q.kind = 1; q.args = &a;
            const int rc = g.meet(tk.idx, q, launcher);
            if (rc < 1 || rc > tk.size || a.first != tk.stream) bad++;                   // a member on another stream than its gang's
        }
        g.leave(tk.idx);
        if (leads) g.wait_empty();
    } else if (hold_us) std::this_thread::sleep_for(std::chrono::microseconds(hold_us));
    c.owner[tk.slot].fetch_sub(1);
    if (leads) { d.stream_owner[(size_t)tk.stream].fetch_sub(1); d.held.fetch_sub(1); }
    gate.release(tk.slot);
}

static int check_order(Dev& d, const char* what) {
    std::sort(d.order.begin(), d.order.end());
    int bad = 0;
    for (size_t i = 1; i < d.order.size(); i++)
        if (d.order[i].first == d.order[i - 1].first || d.order[i].second <= d.order[i - 1].second) bad++;
    printf("%s: %zu leads waited for a stream, %d served out of turn\n", what, d.order.size(), bad);
    return bad;
}

static int hammer_device() {
    Dev d0, d1;
    Ctx A(16, 1, 0), B(32, 2, 0), C(4, 1, 0), D(8, 1, 1);
    A.gate->attach(d0.sched.get()); B.gate->attach(d0.sched.get()); C.gate->attach(d0.sched.get()); D.gate->attach(d1.sched.get());
    A.gate->configure(16, 16, 1, 0);
    B.gate->configure(32, 16, 2, 200);
    C.gate->configure(4, 4, 1, 0);
    D.gate->configure(8, 8, 1, 0);
    std::atomic<int> bad{0}, finished{0}, c_left{8}, detached{0}, ready{0};
    if (d0.sched->read(false).contexts != 3 || d1.sched->read(false).contexts != 1) bad++;
    constexpr int ROUNDS = 60, C_ROUNDS = 20;
    std::vector<std::thread> th;
    auto spawn = [&](Ctx& c, Dev& d, int threads, int rounds, bool gangs, bool is_c) {
        for (int t = 0; t < threads; t++)
            th.emplace_back([&, t, rounds, gangs, is_c] {
                start_together(ready, 96);
                for (int r = 0; r < rounds; r++) one_proof(c, d, gangs && (r + t) % 9 != 0, bad, 300);
                if (is_c && c_left.fetch_sub(1) == 1) {
                    // the last caller of C takes its context off the device while A and B prove on
                    const uint32_t before = d0.sched->read(false).contexts;
                    c.gate->detach();
                    const uint32_t after = d0.sched->read(false).contexts;
                    if (before != 3 || after != 2 || c.gate->attached()) bad++;
                    // ... and goes on with a budget of its own, which the device does not see
                    c.gate->configure(4, 4, 1, 0);
                    const SlotGate::Ticket tk = c.gate->acquire();
                    int own = 0;
                    if (c.gate->load(&own) != 1 || own != 1 || tk.stream != 0) bad++;
                    c.gate->release(tk.slot);
                    detached++;
                }
                finished++;
            });
    };
    spawn(A, d0, 32, ROUNDS, false, false);
    spawn(B, d0, 40, ROUNDS, true, false);
    spawn(C, d0, 8, C_ROUNDS, false, true);
    spawn(D, d1, 16, ROUNDS, false, false);
    join_all(th, finished, "device scheduler");
    const DeviceSched::Counts k0 = d0.sched->read(false), k1 = d1.sched->read(false);
    if (k0.streams_in_use || k0.proofs_in_flight || k0.waiting || k0.contexts != 2) bad++;          // consistent after the detach
    if (k0.streams_peak > (uint32_t)MAX_STREAMS || k0.proofs_peak <= (uint32_t)MAX_STREAMS) bad++;    // (52 slots on 16 streams)
    // the second ordinal: one context of 8 slots - it never saw more, whatever ran on the first
    if (k1.streams_in_use || k1.proofs_in_flight || k1.waiting || k1.contexts != 1 || k1.streams_peak > 8 || k1.proofs_peak > 8) bad++;
    if (A.gate->busy() || B.gate->busy() || D.gate->busy() || A.gate->streams() || B.gate->streams() || detached.load() != 1) bad++;
    if (d0.held.load() || d1.held.load()) bad++;
    bad += check_order(d0, "device 0") + check_order(d1, "device 1");
    if (d0.order.empty()) { printf("no lead ever waited for a stream: the order was not exercised\n"); bad++; }
    if (!d1.order.empty()) bad++;                                                                     // (8 slots on 16 streams: nobody waits)
    const DeviceSched::Counts r0 = d0.sched->read(true);
    if (d0.sched->read(false).streams_peak != 0 || d0.sched->read(false).proofs_peak != 0 || r0.streams_peak == 0) bad++;   // reset
    printf("3 + 1 gates on 2 schedulers, 96 threads: %d + %d + %d + %d proofs, %d ganged on B, peaks %u streams / %u proofs, %d violations\n",
           A.proofs.load(), B.proofs.load(), C.proofs.load(), D.proofs.load(), B.ganged.load(), k0.streams_peak, k0.proofs_peak, bad.load());
    if (A.proofs != 32 * ROUNDS || B.proofs != 40 * ROUNDS || C.proofs != 8 * C_ROUNDS || D.proofs != 16 * ROUNDS) bad++;
    return bad.load();
}

// deterministic: five callers of A parked inside their "proofs", then one caller of C reads the load
static int load_is_the_devices() {
    Dev d;
    Ctx A(16, 1, 0), C(4, 1, 0);
    A.gate->attach(d.sched.get()); C.gate->attach(d.sched.get());
    A.gate->configure(16, 16, 1, 0);
    C.gate->configure(4, 4, 1, 0);
    std::atomic<int> go{0}, finished{0};
    int bad = 0;
    std::vector<std::thread> th;
    for (int t = 0; t < 5; t++)
        th.emplace_back([&] {
            const SlotGate::Ticket tk = A.gate->acquire();
            while (!go.load()) std::this_thread::sleep_for(std::chrono::microseconds(200));
            A.gate->release(tk.slot);
            finished++;
        });
    while (A.gate->busy() != 5) std::this_thread::sleep_for(std::chrono::microseconds(200));
    const SlotGate::Ticket tk = C.gate->acquire();
    int own = 0;
    if (C.gate->load(&own) != 6 || own != 1 || C.gate->busy() != 1) bad++;       // C's one caller sees A's five
    if (A.gate->load(&own) != 6 || own != 5) bad++;
    if (tk.stream != 5) bad++;                                                    // the device's lowest free id, not C's own first
    const DeviceSched::Counts k = d.sched->read(false);
    if (k.contexts != 2 || k.streams_in_use != 6 || k.proofs_in_flight != 6 || k.waiting != 0) bad++;
    C.gate->release(tk.slot);
    go = 1;
    join_all(th, finished, "load figure");
    if (d.sched->read(false).proofs_in_flight != 0) bad++;
    printf("load figure: one caller of C beside five of A reads 6, %d violations\n", bad);
    return bad;
}

// two ganging contexts (32 slots, pairs) on one device: `callers` each
static int two_ganging_contexts(int callers, bool expect_gangs) {
    Dev d;
    Ctx G1(32, 2, 0), G2(32, 2, 0);
    G1.gate->attach(d.sched.get()); G2.gate->attach(d.sched.get());
    G1.gate->configure(32, 16, 2, 200);
    G2.gate->configure(32, 16, 2, 200);
    std::atomic<int> bad{0}, finished{0}, ready{0};
    std::vector<std::thread> th;
    for (int t = 0; t < 2 * callers; t++)
        th.emplace_back([&, t] {
            start_together(ready, 2 * callers);
            for (int r = 0; r < 80; r++) one_proof(t & 1 ? G2 : G1, d, true, bad, 200);
            finished++;
        });
    join_all(th, finished, "two ganging contexts");
    const int ganged = G1.ganged.load() + G2.ganged.load();
    const DeviceSched::Counts k = d.sched->read(false);
    if (k.streams_peak > (uint32_t)MAX_STREAMS || k.streams_in_use || k.proofs_in_flight || k.waiting) bad++;
    if (expect_gangs ? (G1.ganged.load() == 0 || G2.ganged.load() == 0) : ganged != 0) bad++;
    bad += check_order(d, expect_gangs ? "16 + 16 callers" : "8 + 8 callers");
    printf("two ganging contexts, %d + %d callers on %d streams: %d of %d proofs ganged (%s), peak %u streams, %d violations\n", callers, callers,
           MAX_STREAMS, ganged, G1.proofs.load() + G2.proofs.load(), expect_gangs ? "gangs expected in both" : "none expected", k.streams_peak, bad.load());
    return bad.load();
}

int main() {
    int bad = 0;
    bad += load_is_the_devices();
    bad += hammer_device();
    bad += two_ganging_contexts(16, true);
    bad += two_ganging_contexts(8, false);
    if (bad) { printf("SCHED HAMMER FAILED: %d violations\n", bad); return 1; }
    printf("SCHED HAMMER OK\n");
    return 0;
}
