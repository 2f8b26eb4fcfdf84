// walkbatch.h -- one launch for the latency-bound work of every tile that is ready.
//
// A tile's depth-first replay (k_dfs_pool) and its pass loop (k_small_loop) are a few hundred lone
// wavefronts each: one tile's worth leaves the GPU nearly empty, so many tiles must be resident in
// such a phase at once.  Giving every tile a stream of its own buys that only while the process has
// a hardware queue per stream; streams that share a queue run their kernels one after another.
// Here the worker that reaches such a phase SUBMITS its job and blocks.  A submitter that finds a
// walker stream free becomes the LEADER: it takes every pending job of its class, its own included
// (up to the class's caps), launches them as one kernel, waits for it and wakes the members.  While
// all walker streams are busy the arrivals accumulate and the next leader takes them all; with many
// streams a batch shrinks to one job.  Nothing lingers and no timer runs: a submitted job is either
// in a launched batch or has a live thread (its own) that becomes its leader when a stream frees.
//
// No GPU types in here: the launch is a callable, so that a host-only program can drive the batcher
// (tests/native/walkbatch_host.cpp).
#pragma once
#include <stddef.h>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <vector>

namespace walkbatch {

enum { CLS_REPLAY = 0, CLS_LOOP = 1, NCLS = 2 };

struct Job {
    int cls = 0;
    unsigned blocks = 0;        // workgroups of this job
    void *arg = nullptr;        // the launch callable's record of the job
    int launch_rc = 0;          // != 0: the batch's launch failed (every member gets the same)
    char msg[224] = {0};        // ... and why
    double ms = 0.0;            // this job's share of the batch's elapsed time
    bool taken = false;         // in a batch that is out (set and read under the batcher's lock)
    bool done = false;
};

// max_jobs: jobs per launch.  max_blocks: workgroups per launch (a job larger than that still goes, alone).
// budget: jobs of the class in flight at once over ALL launches, direct ones included (0 = no such rule):
// the co-residency rule of the pass loop's grid barriers.
struct Caps { int max_jobs = 1; unsigned max_blocks = ~0u; int budget = 0; };
// blocks: workgroups summed over all launches.  most_blocks: the most workgroups one launch carried.
struct Stats { unsigned long long launches = 0, jobs = 0, largest = 0, blocks = 0, most_blocks = 0; };

class Batcher {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Job *> pending[NCLS];
    int streams_free = 1;
    Caps caps[NCLS];
    int used[NCLS] = {0, 0};            // jobs in flight (only kept against `budget`)
    Stats st[NCLS];

    int budget_free(int cls) const { return caps[cls].budget > 0 ? caps[cls].budget - used[cls] : 0x7fffffff; }
    void count(int cls, int n, unsigned blocks)
    {
        st[cls].launches++;
        st[cls].jobs += (unsigned long long)n;
        if ((unsigned long long)n > st[cls].largest) st[cls].largest = (unsigned long long)n;
        st[cls].blocks += blocks;
        if (blocks > st[cls].most_blocks) st[cls].most_blocks = blocks;
    }

public:
    // (before the first job is submitted)
    void set_streams(int n) { std::lock_guard<std::mutex> lk(mu); streams_free = n < 1 ? 1 : n; }
    void set_caps(int cls, const Caps &c)
    {
        std::lock_guard<std::mutex> lk(mu);
        caps[cls] = c;
        if (caps[cls].max_jobs < 1) caps[cls].max_jobs = 1;
    }

    // Submit the job and return when it has run.  launch(cls, jobs, n, &elapsed_ms, msg, msgcap) runs n jobs of
    // one class to completion on a walker stream and returns 0, or an error code with its text in msg.
    template <class Launch> void run(Job *j, Launch &&launch)
    {
        const int cls = j->cls;
        std::unique_lock<std::mutex> lk(mu);
        pending[cls].push_back(j);
        for (;;) {
            if (j->done) return;            // somebody else's batch carried it
            if (!j->taken && streams_free > 0 && budget_free(cls) >= 1) break;
            cv.wait(lk);            // (taken: its batch is out, the leader will mark it done and notify)
        }
        // leader: its own job first, then the class's pending jobs in order of arrival
        std::vector<Job *> batch;
        j->taken = true;
        batch.push_back(j);
        unsigned blocks = j->blocks;
        int room = budget_free(cls);
        room = room < caps[cls].max_jobs ? room : caps[cls].max_jobs;
        std::deque<Job *> &q = pending[cls];
        for (size_t i = 0; i < q.size();) {
            if (q[i] == j) { q.erase(q.begin() + (long)i); continue; }
            if ((int)batch.size() < room && blocks + q[i]->blocks <= caps[cls].max_blocks) {
                blocks += q[i]->blocks;
                q[i]->taken = true;
                batch.push_back(q[i]);
                q.erase(q.begin() + (long)i);
                continue;
            }
            i++;
        }
        const int n = (int)batch.size();
        streams_free--;
        used[cls] += n;
        count(cls, n, blocks);
        lk.unlock();
        double ms = 0.0;
        char msg[sizeof(j->msg)] = {0};
        const int rc = launch(cls, (Job *const *)batch.data(), n, &ms, msg, sizeof(msg));
        lk.lock();
        for (Job *m : batch) {
            m->launch_rc = rc;
            if (rc) for (size_t c = 0; c < sizeof(msg); c++) m->msg[c] = msg[c];
            m->ms = ms / (double)n;
            m->done = true;
        }
        streams_free++;
        used[cls] -= n;
        lk.unlock();
        cv.notify_all();
    }

    // a one-job launch on the caller's own stream (a context that owns its stream never waits for a batch):
    // it counts against the budget and in the statistics like a batch of one job of `blocks` workgroups
    void direct_begin(int cls, unsigned blocks)
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return budget_free(cls) >= 1; });
        used[cls]++;
        count(cls, 1, blocks);
    }
    void direct_end(int cls)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            used[cls]--;
        }
        cv.notify_all();
    }

    Stats stats(int cls, bool reset)
    {
        std::lock_guard<std::mutex> lk(mu);
        const Stats s = st[cls];
        if (reset) st[cls] = Stats();
        return s;
    }
    int in_flight(int cls) { std::lock_guard<std::mutex> lk(mu); return used[cls]; }
    int waiting(int cls) { std::lock_guard<std::mutex> lk(mu); return (int)pending[cls].size(); }
};

}  // namespace walkbatch
