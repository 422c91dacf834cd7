// host_streams.h - the streams of one context and the record of which of them may hold work (host side of nhdfit.hip).
//
// A context owns four streams: one per pipe (pipe 0 carries everything that is not a step of a staged batch - single finds, mode B,
// uploads, deltas, commits) and the reduce stream of sharded runs.  Whoever is about to touch the node mirror, the staged batch or a
// host block has to know whether a stream may still be working on it, and asking the runtime costs ~3 us per stream (a wait ~10 us: a
// tenth, a third of the scheduler's one-pod calls).  So the answer is kept here, and kept by construction: the handles are private,
// use(k) is the only way to one and marks stream k, wait(k) is the only thing that clears the mark.  An enqueue the ledger does not
// see does not compile.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>

namespace nhdfit {

constexpr int kPipes = 3;           // pipelines a context owns; a staged batch deals its steps to two of them, or to all three (nhdfit_enqueue_step)
constexpr int kRed = kPipes;        // stream index of the reduce stream: the all-reduce of sharded runs, overlapping the next step launch
constexpr int kStreams = kPipes + 1;

// Waiting for a stream: the runtime's own wait parks the thread on the queue's interrupt, and the wake-up costs tens of
// microseconds - as much as a whole step of the pipelined form, half of what a 20-step region loses at its end, a third of a
// batch call through host buffers.  The scheduler's thread has nothing else to do while its one call is in flight (the reference
// calls FindNode from one thread, nhd/NHDScheduler.py:43,277), so it polls the stream first - for at most kSpinWaitUs, the length of
// the longest ordinary call (a mode-B batch) - and only then goes to sleep on it.
constexpr long kSpinWaitUs = 20000;

class StreamLedger {
public:
    hipError_t create() {
        hipError_t e = hipStreamCreateWithFlags(&s_[kRed], hipStreamNonBlocking);
        for (int k = 0; k < kPipes && e == hipSuccess; ++k) e = hipStreamCreateWithFlags(&s_[k], hipStreamNonBlocking);
        return e;
    }
    void destroy() {
        for (hipStream_t& s : s_) { if (s) (void)hipStreamDestroy(s); s = nullptr; }
        marked_ = 0;
    }
    // the handle of stream k for an enqueue - kernel launch, async copy / fill, event record, wait for an event, collective
    hipStream_t use(int k) { marked_ |= 1u << k; return s_[k]; }
    hipError_t wait(int k) {
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t e;
        for (uint32_t polls = 0;; ++polls) {
            e = hipStreamQuery(s_[k]);
            if (e != hipErrorNotReady) {
                if (polls && e == hipSuccess) (void)hipGetLastError();      // ("not ready" must not be what the next launch's error check finds)
                break;
            }
            if ((polls & 63u) == 63u && std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > kSpinWaitUs) {
                (void)hipGetLastError();
                e = hipStreamSynchronize(s_[k]);
                break;
            }
        }
        if (e == hipSuccess) marked_ &= ~(1u << k);
        return e;
    }
    bool clean(int k) const { return !(marked_ >> k & 1u); }
    bool all_clean() const { return marked_ == 0; }
    bool sides_clean() const { return !(marked_ & ~1u); }      // every stream but pipe 0's
    // The one place where the host learns without asking the runtime that pipe 0 has drained: the single-launch find of a batch saw the
    // word its launch stores last, behind everything the call put on the stream.  (The launch itself may still be retiring.)
    void pipe0_drained_by_its_last_word() { marked_ &= ~1u; }
#ifdef NHDFIT_TUNING
    hipError_t query(int k) const { return hipStreamQuery(s_[k]); }      // the tuning build's check of a skipped wait
#endif
private:
    hipStream_t s_[kStreams] = {};
    uint32_t marked_ = 0;           // bit k: something was enqueued on stream k since it was last waited for
};

}  // namespace nhdfit
