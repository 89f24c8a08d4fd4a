// Which proving slot a caller gets, how many are taken, and who proves together: the piece of the backend's host-side threading that
// has no GPU in it, kept on its own so that the sanitizer tier (tools/san/host_hammer.cpp, `make SAN=thread`) runs exactly this code.
//
// A context has `n` slots (one workspace each); up to `max_streams` HIP streams run at a time (16 is the measured optimum at
// 2^17; more cost a few percent: profiles/r06_gang_sweep.txt) - on the DEVICE, over every context attached to its scheduler
// (device_sched.h, attach()); a gate that is not attached keeps a budget of its own.  A caller takes a slot; callers beyond the slots wait their turn (SURVEY.md
// section 8b: "safe to call concurrently from several goroutines").  The busy count is what the load-dependent kernel forms are
// chosen from (backend_impl.h run_msm_body / run_ntt_batch / tail_fill).
//
// Gangs (round 6, gang.h): when MORE callers are in the system than the context has streams, callers are paired up - a "lead" that
// owns a stream and up to gang_max - 1 "followers" that prove on the lead's stream in lockstep.  A lead that has to wait for a free
// stream anyway collects followers for free while it waits; one that finds a stream at once waits at most `wait_us` for partners
// (under sustained load they arrive within microseconds: the callers of a finished gang come back together).  With no more callers
// than streams nobody is ever ganged and nobody ever waits: a lone proof's latency is what it was.
#pragma once
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "device_sched.h"

namespace apk {

class SlotGate {
  public:
    struct Ticket {
        size_t slot = 0;   // the caller's own workspace
        size_t lead = 0;   // the slot whose stream it proves on (== slot when it leads or proves alone)
        int idx = 0;       // member number inside the gang (0 = lead)
        int size = 1;      // members of the gang when it started
        uint64_t gen = 0;  // distinguishes successive gangs of the same lead slot
        int stream = 0;    // which of the device's (unattached: the context's) max_streams streams the gang runs on (a lead's / a lone caller's own)
        uint64_t waited = 0;   // (a lead's) its place among the leads that had to wait for a stream of the device; 0 = it never waited
        uint64_t served = 0;   // (a lead's) the how-manieth stream the scheduler handed out
    };

    SlotGate() {}
    ~SlotGate() { detach(); }
    SlotGate(const SlotGate&) = delete;
    SlotGate& operator=(const SlotGate&) = delete;

    // From here on the gate takes its streams from `s`, counts its callers into it and reads the device's load from it
    // (device_sched.h).  Only while nobody is inside the gate: before configure(), at context creation.  `s` outlives the gate.
    void attach(DeviceSched* s) {
        detach();
        if (!s) return;
        std::lock_guard<std::mutex> lk(s->mu_);
        d_ = s;
        s->contexts_++;
    }
    // back to a private budget; only while none of this gate's slots is held
    void detach() {
        if (d_ == &own_) return;
        DeviceSched* s = d_;
        {
            std::lock_guard<std::mutex> lk(s->mu_);
            s->contexts_--;
            d_ = &own_;
        }
        s->cv_.notify_all();
    }
    bool attached() const { return d_ != &own_; }

    void resize(size_t n) { configure(n, n, 1, 0); }
    void configure(size_t n, size_t max_streams, int gang_max, int wait_us) {
        std::lock_guard<std::mutex> lk(d_->mu_);
        busy_.assign(n, 0); holds_stream_.assign(n, 0); count_.assign(n, 0); size_.assign(n, 0); gen_.assign(n, 0); target_.assign(n, 2);
        taken_ = 0; streams_ = 0; open_lead_ = NONE;
        if (d_ == &own_) own_.set_budget(max_streams);      // (an attached gate runs on the device's budget, whatever it asks for)
        gang_max_ = gang_max < 1 ? 1 : gang_max;
        wait_us_ = wait_us < 0 ? 0 : wait_us;
    }
    size_t size() const { return busy_.size(); }
    int gang_max() const { return gang_max_; }

    // index of a free slot with a stream of its own, taken; blocks while all are busy.  Never ganged (primitives, setup).
    Ticket acquire() { return acquire_member(false); }

    // a proof's way in.  allow_gang = false: as acquire().
    Ticket acquire_member(bool allow_gang) {
        DeviceSched& d = *d_;
        std::unique_lock<std::mutex> lk(d.mu_);
        const bool gangs = allow_gang && gang_max_ > 1;
        size_t i = NONE;
        for (;;) {
            if (gangs && open_lead_ != NONE) {
                i = free_slot();
                if (i != NONE) {       // ---- follower: join the open gang (of THIS context: members share its tables and workspace)
                    take(i);
                    const size_t lead = open_lead_;
                    const uint64_t g0 = gen_[lead];
                    Ticket t;
                    t.slot = i; t.lead = lead; t.idx = count_[lead]++;
                    if (count_[lead] >= target_[lead]) open_lead_ = NONE;  // full: closed to further joins, started by its lead
                    d.cv_.notify_all();
                    d.cv_.wait(lk, [&] { return gen_[lead] != g0; });      // ... until the lead starts it
                    t.size = size_[lead]; t.gen = gen_[lead]; t.stream = holds_stream_[lead] - 1;
                    return t;
                }
            }
            i = free_slot();
            if (i != NONE) break;
            d.waiting_++; d.outside_++;
            d.cv_.wait(lk);
            d.waiting_--; d.outside_--;
        }
        // ---- lead (or alone)
        take(i);
        count_[i] = 1;
        // more callers in the system - on the DEVICE, over every attached context - than streams?  (taken_ counts this caller)
        const bool crowded = gangs && (size_t)(d.taken_ + d.waiting_) > d.max_streams_;
        if (crowded && open_lead_ == NONE) {
            open_lead_ = i;
            // as many members as it takes to put every caller in the system (in flight, or waiting for a slot) on one of the
            // streams: 32 callers on 16 streams prove in pairs even where gangs of four are allowed - sixteen streams of two
            // keep more of the device busy than eight of four
            const size_t in_system = (size_t)(d.taken_ + d.outside_);
            int want = (int)((in_system + d.max_streams_ - 1) / d.max_streams_);
            target_[i] = want < 2 ? 2 : (want > gang_max_ ? gang_max_ : want);
        }
        // (system_clock: libstdc++ then waits with pthread_cond_timedwait, which ThreadSanitizer intercepts - a steady_clock deadline
        // goes through pthread_cond_clockwait, which gcc 11's libtsan does not know, and every later wait is then misreported;
        // a clock step during these few hundred microseconds only shortens or lengthens one wait for partners)
        const auto deadline = std::chrono::system_clock::now() + std::chrono::microseconds(wait_us_);
        uint64_t waited = 0;       // this lead's place in the device's queue, once it has had to wait for a stream
        for (;;) {
            const bool have_stream = d.stream_free_for(waited);
            const bool collecting = open_lead_ == i;       // still open to joins
            if (have_stream && (!collecting || std::chrono::system_clock::now() >= deadline)) break;
            if (!have_stream && !waited) waited = d.enqueue();
            d.waiting_++;
            if (have_stream) d.cv_.wait_until(lk, deadline); else d.cv_.wait(lk);
            d.waiting_--;
        }
        if (open_lead_ == i) open_lead_ = NONE;
        streams_++;
        // the lowest free stream: a device only ever touches max_streams streams, whichever slots of whichever context lead (every
        // further stream is a further hardware queue, and the device time-slices queues beyond what it has: 32 slots leading on
        // 32 streams of their own read 357 against 532 proofs/s, with queues starved for up to 90 ms - profiles/r06_gang_streams.txt)
        uint64_t served = 0;
        const int sid = d.take_stream(waited, &served);
        holds_stream_[i] = sid + 1;
        size_[i] = count_[i];
        gen_[i]++;
        d.cv_.notify_all();
        Ticket t;
        t.slot = i; t.lead = i; t.idx = 0; t.size = size_[i]; t.gen = gen_[i]; t.stream = sid; t.waited = waited; t.served = served;
        return t;
    }
    void release(size_t i) {
        DeviceSched& d = *d_;
        {
            std::lock_guard<std::mutex> lk(d.mu_);
            if (busy_[i]) { busy_[i] = 0; taken_--; d.gave_slot(); }
            if (holds_stream_[i]) { d.give_stream(holds_stream_[i] - 1); holds_stream_[i] = 0; streams_--; }
        }
        d.cv_.notify_all();
    }
    // slots of THIS context in use right now (the caller's own included)
    int busy() {
        std::lock_guard<std::mutex> lk(d_->mu_);
        return taken_;
    }
    // slots in use on the DEVICE, over every context attached to its scheduler (unattached: busy()); *own: this context's share
    int load(int* own = nullptr) {
        std::lock_guard<std::mutex> lk(d_->mu_);
        if (own) *own = taken_;
        return d_->taken_;
    }
    int streams() {
        std::lock_guard<std::mutex> lk(d_->mu_);
        return (int)streams_;
    }
  private:
    static constexpr size_t NONE = (size_t)-1;
    size_t free_slot() const {
        for (size_t i = 0; i < busy_.size(); i++) if (!busy_[i]) return i;
        return NONE;
    }
    void take(size_t i) { busy_[i] = 1; taken_++; d_->took_slot(); }
    DeviceSched own_{1, /*fifo=*/false};    // the private budget of a gate that is not attached
    DeviceSched* d_ = &own_;                // whose mutex, condition variable, streams and load figure this gate runs on
    std::vector<char> busy_;
    std::vector<int> holds_stream_;     // per slot: 1 + the stream it holds as a lead / lone caller, 0 = none
    std::vector<int> count_, size_, target_;   // per lead slot: members so far / members at the start / members it closes at
    std::vector<uint64_t> gen_;         // per lead slot: gangs started
    int taken_ = 0;                     // this context's slots taken (the device's count, the waiting callers: DeviceSched)
    size_t streams_ = 0;                // streams this context's leads hold
    size_t open_lead_ = NONE;
    int gang_max_ = 1, wait_us_ = 0;
};

}  // namespace apk
