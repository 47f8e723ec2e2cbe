// mcraw_race.h -- one race between the candidates of a launch parameter, as a function of (candidate, milliseconds) samples: no HIP
// in here, so that tests/cpp/race_check.cpp can drive it on any machine.  Who times the launches and for what: mcraw_tune.hip.
// The first launches of a geometry try each candidate SAMPLES times (the minimum counts), the fastest stays; afterwards one launch
// in RECHECK is timed -- the chosen candidate and the others in turn -- into a moving average, and the choice moves when another
// candidate has become the faster one by `margin` (a caller whose buffers change is never left measuring, and one whose buffers
// moved to a place where another candidate wins gets there).
#pragma once

namespace mcraw {

struct Race {
    static constexpr int MAXC = 8, SAMPLES = 2;
    static constexpr unsigned long long RECHECK = 64; // one launch in this many is timed once the choice is made
    const float margin;
    int nc = 0, issued[MAXC] = {0}, done[MAXC] = {0};
    float best[MAXC] = {0.f}; // first samples: the minimum; afterwards a moving average
    int decided = -1, under_way = 0; // under_way: handed out by next(), not yet back through sample()
    unsigned long long launches = 0; // since the decision

    explicit Race(float margin_) : margin(margin_) {}

    void reset(int n) // a new geometry
    {
        for (int k = 0; k < MAXC; k++)
            issued[k] = done[k] = 0, best[k] = 0.f;
        nc = n, launches = 0, under_way = 0;
        decided = n == 1 ? 0 : -1; // (nothing to compare: decided at once, never timed)
    }

    // One finished timing; ms <= 0: the sample was lost (an event that could not be read, a launch that never happened).
    void sample(int k, float ms)
    {
        under_way--;
        if (!(ms > 0.f))
            return;
        if (decided < 0)
            best[k] = done[k] && best[k] < ms ? best[k] : ms;
        else
            best[k] = 0.75f * best[k] + 0.25f * ms;
        done[k]++;
    }

    int current() const { return decided > 0 ? decided : 0; } // (the first candidate while nothing is decided)

    // The candidate the next launch is to run AND time, or -1 = run with current(), untimed.
    int next()
    {
        if (nc <= 1)
            return -1;
        int pick = -1;
        if (decided >= 0) {
            for (int k = 0; k < nc; k++)
                if (done[k] > 0 && best[k] < margin * best[decided]) // (the re-checks say another candidate has become the faster one)
                    decided = k;
            if (++launches % RECHECK == 0 && !under_way)
                pick = static_cast<int>((decided + launches / RECHECK) % nc);
        } else {
            bool all = true;
            for (int k = 0; k < nc; k++) {
                all = all && done[k] >= SAMPLES;
                if (issued[k] < SAMPLES + 1 && (pick < 0 || issued[k] < issued[pick]))
                    pick = k;
            }
            // every sample is in, or nothing can be issued any more and what was issued is in or was lost: decide on what there is
            // (else, with every candidate issued and results still on their way, the caller runs with the first meanwhile)
            if (all || (pick < 0 && !under_way)) {
                decided = 0;
                for (int k = 1; k < nc; k++)
                    if (done[k] && (!done[decided] || best[k] < best[decided]))
                        decided = k;
                return -1;
            }
            if (pick >= 0)
                issued[pick]++;
        }
        under_way += pick >= 0;
        return pick;
    }
};

} // namespace mcraw
