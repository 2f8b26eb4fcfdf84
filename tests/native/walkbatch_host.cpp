// Host-only driver of pyshepseg_amd/csrc/walkbatch.h with a fake launch (tests/test_walk_batch_host.py builds it
// with a sanitizer and runs it).  Twelve threads submit jobs of both classes against one walker stream and
// against two; the first launch holds until every other job has been submitted, so coalescing is certain.
// Rounds with equal workgroup counts per class and rounds with unequal ones, where one replay job is larger than
// the launch's workgroup cap: it runs once and alone, and the leader that skips it still takes what fits behind it.
// Usage: walkbatch_host        exit 0 and "ok" when every assertion held
#include "../../pyshepseg_amd/csrc/walkbatch.h"
#include <atomic>
#include <chrono>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <unistd.h>

using namespace walkbatch;

#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) { fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); _exit(1); } \
    } while (0)

static const int NTHREADS = 12, REPLAY_BLOCKS = 30, LOOP_BLOCKS = 64;
static const int REPLAY_MAX_JOBS = 4, LOOP_BUDGET = 3;
static const unsigned REPLAY_MAX_BLOCKS = 100;      // three replays of 30 workgroups: the block cap binds before the job cap
static const int FAIL_LAUNCH_JOB = 5, FAIL_SELF_JOB = 8, LAUNCH_RC = 7;
// the unequal rounds: job i's workgroups (even i: replays, job 4 above the cap; odd i: pass loops)
static const unsigned UNEVEN_BLOCKS[NTHREADS] = {10, 64, 45, 1, 130, 13, 50, 24, 5, 64, 40, 7};
static const int OVERSIZED_JOB = 4;

struct Rec {                // what the fake launch knows about a job
    int id = 0, cls = 0;
    std::atomic<int> runs{0};
    int batch = -1;         // index of the launch that carried it
    bool self_fail = false; // a per-job failure, as a pass loop's own `fail` word
};

struct Round {
    Batcher b;
    Rec rec[NTHREADS];
    Job job[NTHREADS];
    std::atomic<int> launches{0}, completed{0}, loops_in_flight{0}, max_loops{0};
    std::atomic<int> streams_in_use{0};
    std::atomic<bool> picked[NTHREADS];         // in a launch that has begun
    std::atomic<unsigned> most[NCLS], most_shared[NCLS];    // workgroups of the largest launch / of one with company
    std::atomic<int> oversized_alone{0};
    bool uneven = false;
    int nstreams = 1;
    bool hold_first = true, check_greedy = false;
    int failed_batch = -1;
    std::mutex mu;          // failed_batch, batch of a record

    Round()
    {
        for (int i = 0; i < NTHREADS; i++) picked[i] = false;
        for (int c = 0; c < NCLS; c++) { most[c] = 0; most_shared[c] = 0; }
    }
    static void raise(std::atomic<unsigned> &a, unsigned v)
    {
        unsigned m = a.load();
        while (v > m && !a.compare_exchange_weak(m, v)) { }
    }

    int launch(int cls, Job *const *jobs, int n, double *ms, char *msg, size_t cap)
    {
        const int me = launches.fetch_add(1);
        REQUIRE(streams_in_use.fetch_add(1) + 1 <= nstreams);       // as many launches out as there are streams
        REQUIRE(n >= 1);
        unsigned blocks = 0;
        bool fail_launch = false;
        for (int i = 0; i < n; i++) {
            Rec *r = (Rec *)jobs[i]->arg;
            REQUIRE(jobs[i]->cls == cls && r->cls == cls);          // no batch mixes classes
            blocks += jobs[i]->blocks;
            fail_launch |= r->id == FAIL_LAUNCH_JOB;
            REQUIRE(!picked[r->id].exchange(true));                 // no job is in two launches
            if (cls == CLS_REPLAY && jobs[i]->blocks > REPLAY_MAX_BLOCKS) {
                REQUIRE(n == 1);                                    // a job above the block cap goes alone
                oversized_alone.fetch_add(1);
            }
        }
        raise(most[cls], blocks);
        if (n > 1) raise(most_shared[cls], blocks);
        if (cls == CLS_REPLAY) REQUIRE(n <= REPLAY_MAX_JOBS && (n == 1 || blocks <= REPLAY_MAX_BLOCKS));
        else REQUIRE(n <= LOOP_BUDGET);
        if (cls == CLS_LOOP) {
            const int now = loops_in_flight.fetch_add(n) + n;
            REQUIRE(now <= LOOP_BUDGET);                            // the residency budget, direct launches included
            int m = max_loops.load();
            while (now > m && !max_loops.compare_exchange_weak(m, now)) { }
        }
        if (me == 0 && hold_first) {
            // hold until every other job is waiting or done (one inside the other stream's launch is soon done):
            // what follows must coalesce
            for (;;) {
                const int seen = completed.load() + n + b.waiting(CLS_REPLAY) + b.waiting(CLS_LOOP);
                if (seen >= NTHREADS) break;
                std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
        } else if (check_greedy) {
            // one stream, everybody has submitted: a batch that is not full left nothing of its class behind
            const int full = cls == CLS_REPLAY ? (int)(REPLAY_MAX_BLOCKS / REPLAY_BLOCKS) : LOOP_BUDGET;
            if (!uneven) REQUIRE(n == full || b.waiting(cls) == 0);
            // whatever the workgroup counts: every job of the class is pending or was launched by now, and a
            // pending one was left behind only because the batch had no room for it.  A job that did not fit
            // (the oversized one) does not end the leader's scan: what fits behind it is taken
            const unsigned max_blocks = cls == CLS_REPLAY ? REPLAY_MAX_BLOCKS : ~0u;
            const int max_jobs = cls == CLS_REPLAY ? REPLAY_MAX_JOBS : LOOP_BUDGET;
            for (int k = 0; k < NTHREADS; k++)
                if (job[k].cls == cls && !picked[k].load())
                    REQUIRE(n == max_jobs || (unsigned long long)blocks + job[k].blocks > max_blocks);
        }
        std::this_thread::sleep_for(std::chrono::microseconds(300));
        {
            std::lock_guard<std::mutex> lk(mu);
            for (int i = 0; i < n; i++) {
                Rec *r = (Rec *)jobs[i]->arg;
                r->runs.fetch_add(1);
                r->batch = me;
                if (r->id == FAIL_SELF_JOB) r->self_fail = true;
            }
            if (fail_launch) failed_batch = me;
        }
        if (cls == CLS_LOOP) loops_in_flight.fetch_sub(n);
        completed.fetch_add(n);
        streams_in_use.fetch_sub(1);
        *ms = 1.5 * n;
        if (fail_launch) { snprintf(msg, cap, "fake launch %d failed", me); return LAUNCH_RC; }
        return 0;
    }
};

static void run_round(int nstreams, bool hold, int ndirect, bool uneven = false)
{
    Round *R = new Round();
    R->uneven = uneven;
    R->nstreams = nstreams;
    R->hold_first = hold;
    R->check_greedy = hold && nstreams == 1;
    R->b.set_streams(nstreams);
    Caps c0, c1;
    c0.max_jobs = REPLAY_MAX_JOBS; c0.max_blocks = REPLAY_MAX_BLOCKS; c0.budget = 0;
    c1.max_jobs = LOOP_BUDGET; c1.max_blocks = ~0u; c1.budget = LOOP_BUDGET;
    R->b.set_caps(CLS_REPLAY, c0);
    R->b.set_caps(CLS_LOOP, c1);
    std::vector<std::thread> th;
    for (int i = 0; i < NTHREADS; i++) {
        R->rec[i].id = i;
        R->rec[i].cls = i & 1;
        R->job[i].cls = i & 1;
        R->job[i].blocks = uneven ? UNEVEN_BLOCKS[i] : (i & 1) ? (unsigned)LOOP_BLOCKS : (unsigned)REPLAY_BLOCKS;
        R->job[i].arg = &R->rec[i];
    }
    for (int i = 0; i < NTHREADS; i++) {
        th.emplace_back([R, i, ndirect] {
            if (i < ndirect) {
                // a context that owns its stream: a launch of its own, counted against the same budget
                const int cls = R->job[i].cls;
                R->b.direct_begin(cls, R->job[i].blocks);
                REQUIRE(!R->picked[i].exchange(true));
                Round::raise(R->most[cls], R->job[i].blocks);
                if (cls == CLS_LOOP) REQUIRE(R->loops_in_flight.fetch_add(1) + 1 <= LOOP_BUDGET);
                std::this_thread::sleep_for(std::chrono::microseconds(300));
                R->rec[i].runs.fetch_add(1);
                if (cls == CLS_LOOP) R->loops_in_flight.fetch_sub(1);
                R->completed.fetch_add(1);
                R->b.direct_end(cls);
                R->job[i].done = true;
                return;
            }
            R->b.run(&R->job[i], [R](int cls, Job *const *jobs, int n, double *ms, char *msg, size_t cap) {
                return R->launch(cls, jobs, n, ms, msg, cap);
            });
        });
    }
    for (auto &t : th) t.join();
    unsigned long long jobs_seen = 0, launches_seen = 0;
    for (int c = 0; c < NCLS; c++) {
        const Stats s = R->b.stats(c, false);
        jobs_seen += s.jobs; launches_seen += s.launches;
        REQUIRE(s.jobs == (unsigned long long)NTHREADS / 2 && s.launches <= s.jobs && s.largest >= 1);
        if (R->check_greedy) REQUIRE(s.largest >= 2);              // the batch after the held one coalesced
        REQUIRE(R->b.in_flight(c) == 0 && R->b.waiting(c) == 0);
        // the workgroup counters: every submitted job's workgroups once, and the largest launch as the fake saw it
        unsigned long long want_blocks = 0;
        for (int i = c; i < NTHREADS; i += 2) want_blocks += R->job[i].blocks;
        REQUIRE(s.blocks == want_blocks);
        REQUIRE(s.most_blocks == R->most[c].load() && s.most_blocks >= 1 && s.most_blocks <= s.blocks);
    }
    // a replay launch above the block cap is a single job
    REQUIRE(R->most_shared[CLS_REPLAY].load() <= REPLAY_MAX_BLOCKS);
    const Stats rs = R->b.stats(CLS_REPLAY, false);
    if (uneven) {
        REQUIRE(rs.most_blocks == UNEVEN_BLOCKS[OVERSIZED_JOB] && UNEVEN_BLOCKS[OVERSIZED_JOB] > REPLAY_MAX_BLOCKS);
        // ... which ran once and alone (directly, or as a launch of one)
        REQUIRE(R->oversized_alone.load() == (OVERSIZED_JOB < ndirect ? 0 : 1));
        REQUIRE(R->rec[OVERSIZED_JOB].runs.load() == 1);
    } else {
        REQUIRE(rs.most_blocks <= REPLAY_MAX_BLOCKS && R->oversized_alone.load() == 0);
    }
    // reset clears every field, the workgroup counters included
    for (int c = 0; c < NCLS; c++) {
        (void)R->b.stats(c, true);
        const Stats z = R->b.stats(c, false);
        REQUIRE(z.launches == 0 && z.jobs == 0 && z.largest == 0 && z.blocks == 0 && z.most_blocks == 0);
    }
    REQUIRE(jobs_seen == (unsigned long long)NTHREADS);
    REQUIRE(launches_seen == (unsigned long long)(R->launches.load() + ndirect));
    for (int i = 0; i < NTHREADS; i++) {
        REQUIRE(R->job[i].done);
        REQUIRE(R->rec[i].runs.load() == 1);                        // every job ran exactly once
        if (i < ndirect) continue;
        // a launch error reaches exactly that batch's members, with its text
        const bool in_failed = R->rec[i].batch == R->failed_batch;
        REQUIRE((R->job[i].launch_rc == LAUNCH_RC) == in_failed);
        if (in_failed) REQUIRE(strstr(R->job[i].msg, "failed") != nullptr);
        else REQUIRE(R->job[i].launch_rc == 0 && R->job[i].msg[0] == 0);
        // a per-job failure reaches only that job
        REQUIRE(R->rec[i].self_fail == (i == FAIL_SELF_JOB));
        REQUIRE(R->job[i].ms == 1.5);                               // an equal share of the batch's time
    }
    if (ndirect <= FAIL_LAUNCH_JOB) REQUIRE(R->failed_batch >= 0);
    REQUIRE(R->max_loops.load() <= LOOP_BUDGET);
    delete R;
}

int main()
{
    alarm(30);                      // the program ends within its own time limit or dies by SIGALRM
    for (int rep = 0; rep < 20; rep++) {
        run_round(1, true, 0);      // one stream, held first launch: everything after it coalesces
        run_round(2, true, 0);      // two streams: the second keeps launching while the first is held
        run_round(1, false, 4);     // no hold, four jobs launched directly: the budget is shared with them
        run_round(2, false, 0);
        // unequal workgroup counts, one replay above the block cap
        run_round(1, true, 0, true);
        run_round(2, true, 0, true);
        run_round(1, false, 6, true);   // the oversized replay among the direct launches
        run_round(2, false, 0, true);
    }
    printf("ok\n");
    return 0;
}
