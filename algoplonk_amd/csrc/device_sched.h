// What belongs to the DEVICE in the host-side scheduling, not to a context: how many proving streams run at a time, which of them
// are taken, how many proofs are in flight and how many callers wait - over every context attached to the device.  GPU-free, like
// slot_gate.h, so that the sanitizer tier (tools/san/sched_hammer.cpp, `make SAN=thread san-sched`) runs exactly this code.
//
// A process that serves several circuits holds several contexts on one GPU.  Each of them used to schedule as if it owned the
// device: 16 streams of its own, kernel forms chosen from its own busy count, gangs judged against its own callers.  One
// DeviceSched per device ordinal (the registry is in apk_api.cpp) now owns
//   - the stream budget: ids 0 .. max_streams - 1 (APK_MAX_SLOTS), handed out lowest-free; the HIP streams behind the ids are
//     created once per device by the backend layer and lent to whichever context's lead holds the id;
//   - the load figure: slots held and callers waiting, over all attached contexts - what the load-dependent kernel forms and the
//     "more callers than streams" test of the gangs are decided from;
//   - one mutex and one condition variable for every attached SlotGate, so that a lead of context A that waits for a stream
//     wakes when context B gives one back;
//   - the order: leads that have to wait for a stream are served in the order they began to wait, whichever context they belong
//     to (a ticket queue) - a context with many callers cannot starve a context with one.
// What stays in the SlotGate is what belongs to a context: its slots (workspaces), its own busy count, its gangs (members share
// the context's tables, MSM workspace and launch shapes, so a gang never spans contexts).
//
// A SlotGate that was never attached carries a private DeviceSched of its own (its max_streams, no queue): it behaves as it did
// before there was a scheduler.
#pragma once
#include <stdint.h>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <vector>

namespace apk {

class DeviceSched {
  public:
    struct Counts {
        uint32_t contexts, max_streams, streams_in_use, streams_peak, proofs_in_flight, proofs_peak, waiting;
    };
    // fifo: leads that wait for a stream are served in ticket order (the device-wide scheduler); false: whoever wakes first (a
    // gate's private budget)
    explicit DeviceSched(size_t max_streams = 1, bool fifo = true) : fifo_(fifo) { set_budget(max_streams); }
    DeviceSched(const DeviceSched&) = delete;
    DeviceSched& operator=(const DeviceSched&) = delete;

    size_t max_streams() {
        std::lock_guard<std::mutex> lk(mu_);
        return max_streams_;
    }
    // the figures of apk_device_sched_read; reset: the peaks start again from what is held now
    Counts read(bool reset) {
        std::lock_guard<std::mutex> lk(mu_);
        Counts c;
        c.contexts = (uint32_t)contexts_; c.max_streams = (uint32_t)max_streams_;
        c.streams_in_use = (uint32_t)streams_; c.streams_peak = (uint32_t)streams_peak_;
        c.proofs_in_flight = (uint32_t)taken_; c.proofs_peak = (uint32_t)taken_peak_;
        c.waiting = (uint32_t)waiting_;
        if (reset) { streams_peak_ = streams_; taken_peak_ = taken_; }
        return c;
    }

  private:
    friend class SlotGate;     // everything below is touched by the attached gates only, with mu_ held
    void set_budget(size_t max_streams) {
        max_streams_ = max_streams < 1 ? 1 : max_streams;
        stream_busy_.assign(max_streams_, 0);
        streams_ = 0; streams_peak_ = 0; taken_ = 0; taken_peak_ = 0; waiting_ = 0; outside_ = 0;
        queue_.clear();
    }
    void took_slot() { if (++taken_ > taken_peak_) taken_peak_ = taken_; }
    void gave_slot() { taken_--; }
    // may a lead take a stream now?  `ticket`: its place in the queue, 0 = it has not had to wait so far
    bool stream_free_for(uint64_t ticket) const {
        if (streams_ >= max_streams_) return false;
        return !fifo_ || queue_.empty() || queue_.front() == ticket;
    }
    uint64_t enqueue() {
        if (!fifo_) return 0;
        queue_.push_back(next_ticket_);
        return next_ticket_++;
    }
    // the lowest free stream id (a device only ever touches max_streams proving streams, whoever leads); *served: the how-manieth
    // stream this scheduler has handed out
    int take_stream(uint64_t ticket, uint64_t* served) {
        if (ticket) queue_.pop_front();      // (stream_free_for(ticket) held: it is the front)
        if (++streams_ > streams_peak_) streams_peak_ = streams_;
        int sid = 0;
        while ((size_t)sid + 1 < stream_busy_.size() && stream_busy_[sid]) sid++;
        stream_busy_[sid] = 1;
        *served = ++served_;
        return sid;
    }
    void give_stream(int sid) { stream_busy_[(size_t)sid] = 0; streams_--; }

    std::mutex mu_;
    std::condition_variable cv_;
    const bool fifo_;
    size_t max_streams_ = 1, streams_ = 0, streams_peak_ = 0;
    std::vector<char> stream_busy_;
    int taken_ = 0, taken_peak_ = 0;     // slots held over all attached gates (proofs and primitives in flight)
    int waiting_ = 0, outside_ = 0;      // callers waiting inside a gate (with or without a slot); ... without a slot
    int contexts_ = 0;                   // attached gates
    std::deque<uint64_t> queue_;         // tickets of the leads waiting for a stream, oldest first
    uint64_t next_ticket_ = 1, served_ = 0;
};

}  // namespace apk
