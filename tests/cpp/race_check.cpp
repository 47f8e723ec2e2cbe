// race_check.cpp -- csrc/mcraw_race.h on its own (no HIP: that this file compiles with a plain g++ is part of the test): the rule
// of the context's races, checked case by case for 1, 2 and 8 candidates and both margins, and replayed against transcriptions of
// the two functions it replaced (tune_pick and side_pick of mcraw_tune.hip, their events replaced by scripted samples that finish
// in random order).  Prints "wrong N"; every failed check says where.  tests/test_tune_race.py builds and runs it.
#include "mcraw_race.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

using mcraw::Race;

static int wrong = 0;
#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            if (wrong++ < 40)                                                                                          \
                std::printf("%s:%d: nc %d margin %.2f: %s\n", __func__, __LINE__, nc, static_cast<double>(margin), #cond); \
        }                                                                                                              \
    } while (0)

// ---- the rule, case by case

static void one_candidate(float margin)
{
    const int nc = 1;
    Race r(margin);
    r.reset(nc);
    CHECK(r.decided == 0 && r.current() == 0); // decided at once
    for (int i = 0; i < 200; i++)
        CHECK(r.next() == -1); // never timed
    CHECK(r.decided == 0 && r.under_way == 0);
}

static void hand_out_and_cap(int nc, float margin)
{
    Race r(margin);
    r.reset(nc);
    for (int round = 0; round < 3; round++) // least issued first, the lower index on ties
        for (int k = 0; k < nc; k++)
            CHECK(r.next() == k && r.decided == -1 && r.current() == 0);
    for (int i = 0; i < 100; i++) // three issues per candidate and no more; results under way: -1, and nothing is decided
        CHECK(r.next() == -1 && r.decided == -1 && r.current() == 0);
    for (int k = 0; k < nc; k++)
        CHECK(r.issued[k] == 3 && r.done[k] == 0);
    CHECK(r.under_way == 3 * nc);
    // every candidate's second sample but the last one's: still under way, still undecided
    for (int k = 0; k < nc; k++)
        r.sample(k, 5.f), r.sample(k, k == nc - 1 ? 0.f : 4.f); // (the last candidate loses one)
    CHECK(r.next() == -1 && r.decided == -1);
    r.sample(nc - 1, 3.f); // its third issue comes in: every candidate has two samples now
    CHECK(r.decided == -1);
    CHECK(r.next() == -1 && r.decided == nc - 1 && r.current() == nc - 1);
}

static void decision(int nc, float margin)
{
    // samples come back at once.  Candidate k: first sample 12 + k, second 22 - 3 k: the minima are 12, 13, 14, 13, 10, 7, 4, 1 (the
    // first sample for some, the second for others); the smallest is the last candidate's for nc = 8, the first one's for nc = 2
    Race r(margin);
    r.reset(nc);
    float expect_best[Race::MAXC];
    for (int round = 0; round < 2; round++)
        for (int k = 0; k < nc; k++) {
            const int p = r.next();
            CHECK(p == k && r.decided == -1); // (not decided before the last candidate's second sample)
            const float ms = round == 0 ? 12.f + k : 22.f - 3.f * k;
            r.sample(p, ms);
            expect_best[k] = round == 0 ? ms : std::min(expect_best[k], ms);
        }
    CHECK(r.decided == -1); // (the decision is taken by the next call)
    CHECK(r.next() == -1);
    const int win = static_cast<int>(std::min_element(expect_best, expect_best + nc) - expect_best);
    CHECK(r.decided == win && r.current() == win);
    for (int k = 0; k < nc; k++)
        CHECK(r.best[k] == expect_best[k] && r.done[k] == 2 && r.issued[k] == 2);
    // ties go to the lower index
    r.reset(nc);
    for (int i = 0; i < 2 * nc; i++) {
        const int p = r.next();
        r.sample(p, p == 0 ? 9.f : (p == nc - 1 || p == 1) ? 7.f : 8.f);
    }
    CHECK(r.next() == -1 && r.decided == 1);
    r.reset(nc);
    for (int i = 0; i < 2 * nc; i++)
        r.sample(r.next(), 5.f);
    CHECK(r.next() == -1 && r.decided == 0);
}

static void lost_samples(int nc, float margin)
{
    for (int loser : {0, nc - 1}) { // all of one candidate's samples are lost
        Race r(margin);
        r.reset(nc);
        for (int i = 0; i < 3 * nc; i++) {
            const int p = r.next();
            CHECK(p == i % nc && r.decided == -1);
            r.sample(p, p == loser ? 0.f : 10.f - p); // (the later candidates are the faster ones)
        }
        CHECK(r.decided == -1);
        CHECK(r.next() == -1);
        const int win = loser == nc - 1 ? nc - 2 : nc - 1;
        CHECK(r.decided == win && r.done[loser] == 0);
    }
    Race r(margin); // all samples lost, the last one late: candidate 0, once nothing is under way
    r.reset(nc);
    for (int i = 0; i < 3 * nc; i++) {
        const int p = r.next();
        if (i < 3 * nc - 1)
            r.sample(p, i % 2 ? 0.f : -1.f);
    }
    CHECK(r.next() == -1 && r.decided == -1);
    r.sample(nc - 1, 0.f);
    CHECK(r.next() == -1 && r.decided == 0 && r.current() == 0);
}

// A race decided for candidate `win`: every candidate's samples 1.2 ms, the winner's 1.0 ms.
static void decide_for(Race &r, int nc, int win)
{
    r.reset(nc);
    for (int i = 0; i < 2 * nc; i++) {
        const int p = r.next();
        r.sample(p, p == win ? 1.0f : 1.2f);
    }
    r.next();
}

static void rechecks(int nc, float margin)
{
    for (int win : {0, nc - 1}) {
        Race r(margin);
        decide_for(r, nc, win);
        CHECK(r.decided == win);
        // (decide_for's last call was not counted: it took the decision)
        unsigned long long calls = 0;
        for (int q = 1; q <= 2 * nc + 1; q++) {
            for (int i = 0; i < 63; i++, calls++)
                CHECK(r.next() == -1);
            const int p = r.next(); // one launch in 64, the candidates in turn from the chosen one on
            calls++;
            CHECK(p == (win + q) % nc);
            CHECK(r.launches == calls);
            r.sample(p, p == win ? 1.0f : 1.2f);
            CHECK(r.decided == win);
        }
        // a sample that stays under way: no other launch is timed until it is in
        for (int i = 0; i < 63; i++)
            CHECK(r.next() == -1);
        const int held = r.next();
        CHECK(held >= 0);
        for (int i = 0; i < 3 * 64; i++)
            CHECK(r.next() == -1);
        r.sample(held, 0.f); // (lost, and no longer under way)
        for (int i = 0; i < 63; i++)
            CHECK(r.next() == -1);
        CHECK(r.next() == (win + 2 * nc + 1 + 5) % nc);
    }
}

static void average_and_margin(int nc, float margin)
{
    Race r(margin);
    decide_for(r, nc, 0);
    for (int i = 0; i < 63; i++)
        r.next();
    CHECK(r.next() == 1);
    r.sample(1, 0.32f); // 0.75 * 1.2 + 0.25 * 0.32 = 0.98: under 0.99 of the chosen one's 1.0, not under 0.97
    const float avg = 0.75f * 1.2f + 0.25f * 0.32f;
    CHECK(r.best[1] == avg && r.done[1] == 3 && r.decided == 0); // (the choice moves in next(), not in sample())
    CHECK(avg < 0.99f * 1.0f && !(avg < 0.97f * 1.0f));
    r.next();
    CHECK(r.decided == (margin == 0.99f ? 1 : 0));
    // ... and a second one that crosses both.  It is candidate 1's turn again after nc re-checks (the others keep their 1.2)
    int turns = 0;
    for (int i = 0; i < 64 * (nc + 2) && turns < 1; i++) {
        const int p = r.next();
        if (p == 1)
            r.sample(p, 0.5f), turns++;
        else if (p >= 0)
            r.sample(p, p == 0 ? 1.0f : 1.2f);
    }
    CHECK(turns == 1 && r.best[1] == 0.75f * avg + 0.25f * 0.5f);
    r.next();
    CHECK(r.decided == 1 && r.current() == 1);
}

static void reset_forgets(int nc, float margin)
{
    Race r(margin);
    decide_for(r, nc, nc - 1);
    for (int i = 0; i < 64; i++)
        r.next(); // (one sample under way)
    r.reset(nc);
    CHECK(r.decided == -1 && r.launches == 0 && r.under_way == 0 && r.current() == 0 && r.nc == nc);
    for (int k = 0; k < Race::MAXC; k++)
        CHECK(r.issued[k] == 0 && r.done[k] == 0 && r.best[k] == 0.f);
    for (int k = 0; k < nc; k++)
        CHECK(r.next() == k);
    r.reset(1);
    CHECK(r.decided == 0 && r.next() == -1);
}

// ---- the functions the rule replaced, transcribed: the state of an entry, its pending events as scripted samples

struct Scripted {
    int cand;
    float ms; // <= 0: the sample is lost
    bool finished;
};

struct Old {
    int nc = 0, issued[8] = {0}, done[8] = {0};
    float best[8] = {0.f};
    int decided = -1;
    unsigned long long launches = 0;
    std::vector<Scripted> pending;

    void collect() // (both functions' loop over their pending events)
    {
        for (size_t i = 0; i < pending.size();) {
            if (!pending[i].finished) {
                i++;
                continue;
            }
            const float ms = pending[i].ms;
            if (ms > 0.f) {
                const int k = pending[i].cand;
                if (decided < 0)
                    best[k] = done[k] ? std::min(best[k], ms) : ms;
                else
                    best[k] = 0.75f * best[k] + 0.25f * ms;
                done[k]++;
            }
            pending.erase(pending.begin() + static_cast<long>(i));
        }
    }

    int tune_pick() // two candidates, margin 0.99
    {
        constexpr int NC = 2, SAMPLES = 2;
        constexpr unsigned long long RECHECK = 64;
        Old &t = *this;
        if (t.decided >= 0) {
            const int other = 1 - t.decided;
            if (t.best[other] < 0.99f * t.best[t.decided])
                t.decided = other;
            t.launches++;
            if (t.launches % RECHECK != 0 || !t.pending.empty())
                return -1;
            return (t.launches / RECHECK) % 2 ? 1 - t.decided : t.decided;
        }
        bool all = true;
        for (int k = 0; k < NC; k++)
            all = all && t.done[k] >= SAMPLES;
        if (all) {
            t.decided = 0;
            for (int k = 1; k < NC; k++)
                if (t.best[k] < t.best[t.decided])
                    t.decided = k;
            return -1;
        }
        int pick = -1;
        for (int k = 0; k < NC; k++)
            if (t.issued[k] < SAMPLES + 1 && (pick < 0 || t.issued[k] < t.issued[pick]))
                pick = k;
        if (pick < 0)
            return -1;
        t.issued[pick]++;
        return pick;
    }

    int side_pick() // up to eight candidates, margin 0.97
    {
        constexpr int SAMPLES = 2;
        constexpr unsigned long long RECHECK = 64;
        Old &t = *this;
        if (t.nc == 1) {
            t.decided = 0;
            return -1;
        }
        if (t.decided >= 0) {
            for (int k = 0; k < t.nc; k++)
                if (t.done[k] > 0 && t.best[k] < 0.97f * t.best[t.decided])
                    t.decided = k;
            t.launches++;
            if (t.launches % RECHECK != 0 || !t.pending.empty())
                return -1;
            return static_cast<int>((t.launches / RECHECK) % static_cast<unsigned long long>(t.nc));
        }
        bool all_done = true;
        for (int k = 0; k < t.nc; k++)
            all_done = all_done && t.done[k] >= SAMPLES;
        if (all_done) {
            t.decided = 0;
            for (int k = 1; k < t.nc; k++)
                if (t.best[k] < t.best[t.decided])
                    t.decided = k;
            return -1;
        }
        int pick = -1;
        for (int k = 0; k < t.nc; k++)
            if (t.issued[k] < SAMPLES + 1 && (pick < 0 || t.issued[k] < t.issued[pick]))
                pick = k;
        if (pick < 0) {
            if (t.pending.empty()) {
                t.decided = 0;
                for (int k = 1; k < t.nc; k++)
                    if (t.done[k] && (!t.done[t.decided] || t.best[k] < t.best[t.decided]))
                        t.decided = k;
            }
            return -1;
        }
        t.issued[pick]++;
        return pick;
    }
};

// One script: `calls` launches; before each, every sample under way finishes with probability 1/3 (so they come in in any order,
// and re-checks find earlier ones still under way); the candidates' times drift, so that the choice moves now and then.
// `side`: against side_pick, with lost samples, until both have decided; else against tune_pick, no sample lost.
static int moves = 0; // of the choice, after the first decision, in the scripts against tune_pick

static int replay(unsigned seed, int nc, float margin, bool side, int calls)
{
    std::mt19937 rng(seed);
    auto uni = [&]() { return static_cast<float>(rng() >> 8) / 16777216.f; };
    Old old;
    old.nc = nc;
    Race r(margin);
    r.reset(nc);
    float mean[8];
    for (int k = 0; k < nc; k++)
        mean[k] = 1.f + 0.1f * uni();
    int bad = 0;
    for (int i = 0; i < calls; i++) {
        for (Scripted &s : old.pending)
            s.finished = rng() % 3u == 0u;
        for (const Scripted &s : old.pending)
            if (s.finished)
                r.sample(s.cand, s.ms);
        old.collect();
        const int was = old.decided;
        const int po = side ? old.side_pick() : old.tune_pick();
        const int pn = r.next();
        bad += po != pn || old.decided != r.decided || std::max(old.decided, 0) != r.current();
        moves += !side && was >= 0 && old.decided != was;
        if (side && old.decided >= 0)
            break;
        if (po >= 0) {
            const bool lost = side && rng() % 4u == 0u;
            old.pending.push_back({po, lost ? (rng() % 2u ? 0.f : -1.f) : mean[po] * (0.97f + 0.06f * uni()), false});
        }
        if (i % 500 == 499)
            for (int k = 0; k < nc; k++)
                mean[k] = 1.f + 0.1f * uni();
    }
    for (int k = 0; k < nc; k++)
        bad += old.best[k] != r.best[k] || old.done[k] != r.done[k] || old.issued[k] != r.issued[k];
    bad += static_cast<int>(old.pending.size()) != r.under_way || old.decided < 0;
    return bad;
}

int main()
{
    for (float margin : {0.99f, 0.97f}) {
        one_candidate(margin);
        for (int nc : {2, 8}) {
            hand_out_and_cap(nc, margin);
            decision(nc, margin);
            lost_samples(nc, margin);
            rechecks(nc, margin);
            average_and_margin(nc, margin);
            reset_forgets(nc, margin);
        }
    }
    int scripts = 0;
    for (unsigned seed = 1; seed <= 320; seed++, scripts++) {
        if (const int bad = replay(seed, 2, 0.99f, false, 2000)) {
            if (wrong++ < 40)
                std::printf("tune_pick script %u: %d differences\n", seed, bad);
        }
        for (int nc : {3, 8})
            if (const int b = replay(seed, nc, 0.97f, true, 2000)) {
                if (wrong++ < 40)
                    std::printf("side_pick script %u, nc %d: %d differences\n", seed, nc, b);
            }
    }
    if (moves < scripts / 4) { // (a check of the scripts: their drifting times are there to make the choice move)
        std::printf("the choice moved %d times only in %d scripts against tune_pick\n", moves, scripts);
        wrong++;
    }
    std::printf("scripts %d moves %d\nwrong %d\n", scripts, moves, wrong);
    return wrong != 0;
}
