// mapcaller_amd/csrc/mcx_pool.h — the file front end's host threads: a pool that lives as long as the run, a bounded queue between two stages, a clock.
// Nothing of the project's is included: the file compiles alone (tests/hostemu/pool_check.cpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

namespace mcx { namespace files {

typedef std::chrono::steady_clock::time_point Tick;
inline Tick now() { return std::chrono::steady_clock::now(); }
inline double secs(Tick a, Tick b) { return std::chrono::duration<double>(b - a).count(); }

// ---- a pool of host threads that lives as long as the run ---------------------------------------------------
// Every run() publishes one job object; a worker takes hold of it under the mutex and draws indices from that object alone, so a worker that is late for
// one run can neither take a part of the next one nor count against it.
class Pool {
public:
    explicit Pool(int n) : n_(std::max(1, n))
    {
        for (int k = 1; k < n_; k++) th_.emplace_back([this] { work(); });
    }
    ~Pool()
    {
        { std::unique_lock<std::mutex> l(m_); stop_ = true; cv_.notify_all(); }
        for (auto &t : th_) t.join();
    }
    int size() const { return n_; }
    // f(k) for k in [0, parts), the calling thread taking its share; returns when all are done.  One run() at a time per pool.
    void run(int parts, const std::function<void(int)> &f)
    {
        if (parts <= 0) return;
        if (parts == 1 || n_ == 1) { for (int k = 0; k < parts; k++) f(k); return; }
        const std::shared_ptr<Job> j = std::make_shared<Job>(f, parts);
        { std::unique_lock<std::mutex> l(m_); job_ = j; gen_++; cv_.notify_all(); }
        drain(*j);
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [&] { return j->left == 0; });
        job_.reset(); // (f is the caller's: no worker calls it from here on — one that still holds the job finds its indices drawn)
    }
    // slices a range of n items is cut into: at least `grain` items each, at most one per thread
    int slices(uint64_t n, uint64_t grain) const { return (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_, n / grain)); }
    // f(k, lo, hi) for slice k = [lo, hi) of [0, n)
    template <class F> void for_range(uint64_t n, uint64_t grain, const F &f)
    {
        const uint64_t s = (uint64_t)slices(n, grain);
        run((int)s, [&](int k) { f(k, n * (uint64_t)k / s, n * (uint64_t)(k + 1) / s); });
    }
private:
    struct Job {
        Job(const std::function<void(int)> &fn, int n) : f(fn), parts(n), left(n) {}
        const std::function<void(int)> &f; // the caller's, alive until run() returns: called only for an index drawn below `parts`, and run() returns only after all of
                                           // those have finished — a worker that holds the job longer finds `next >= parts` and never touches f (keep it so)
        const int parts;
        std::atomic<int> next{0};
        int left; // parts not finished yet (under the pool's mutex)
    };
    void drain(Job &j)
    {
        for (;;) {
            const int k = j.next.fetch_add(1);
            if (k >= j.parts) break;
            j.f(k);
            std::unique_lock<std::mutex> l(m_);
            if (--j.left == 0) done_.notify_all();
        }
    }
    void work()
    {
        uint64_t seen = 0;
        for (;;) {
            std::shared_ptr<Job> j;
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                j = job_;
            }
            if (j) drain(*j);
        }
    }
    int n_;
    std::vector<std::thread> th_;
    std::mutex m_; std::condition_variable cv_, done_;
    std::shared_ptr<Job> job_;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

template <typename T> class Queue { // bounded hand-over between two stages
public:
    explicit Queue(size_t cap) : cap_(cap) {}
    void push(T v) { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [&] { return q_.size() < cap_; }); q_.push_back(std::move(v)); cv_.notify_all(); }
    T pop() { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [&] { return !q_.empty(); }); T v = std::move(q_.front()); q_.pop_front(); cv_.notify_all(); return v; }
    bool try_pop(T &v) { std::unique_lock<std::mutex> l(m_); if (q_.empty()) return false; v = std::move(q_.front()); q_.pop_front(); cv_.notify_all(); return true; }
private:
    std::mutex m_; std::condition_variable cv_; std::deque<T> q_; size_t cap_;
};

}} // namespace mcx::files
