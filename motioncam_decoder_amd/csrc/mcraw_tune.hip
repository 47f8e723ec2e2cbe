// mcraw_tune.hip -- the context's run-time measurements (host side of the C ABI, see mcraw_host.h): the two races that single
// launches run between events (which XCD mapping k7_tiles runs with, how many parts resolve a long side stream; the rule itself is
// mcraw_race.h), and the two trials of the host-memory pipeline on the host's clock (status words fetched or sent home).
#include "mcraw_host.h"

using namespace mcraw;

namespace mcraw {


// The tuner's entry of a geometry, made the last used one.  A geometry that is new to the tuner takes the entry that was not used
// for the longest time: its race has no candidates (nc == 0) until the caller has given it some.
static Tuner::Entry &entry_of(mcraw_ctx *c, Tuner &t, int n7, uint32_t R, uint32_t mode)
{
    Tuner::Entry *e = nullptr, *lru = &t.entries[0];
    for (Tuner::Entry &x : t.entries) {
        if (x.race.nc && x.key_n == n7 && x.key_R == R && x.key_mode == mode)
            e = &x;
        if (x.used < lru->used)
            lru = &x;
    }
    if (!e) {
        e = lru;
        for (auto &p : e->pending) { // (their results belong to the old geometry)
            (void)hipEventSynchronize(p.b);
            c->event_pool.insert(c->event_pool.end(), {p.a, p.b});
        }
        e->pending.clear();
        e->key_n = n7, e->key_R = R, e->key_mode = mode, e->race.reset(0);
    }
    e->used = ++t.clock;
    return *(t.last = e);
}

// Which candidate of the entry the next launch runs with; `tm` times it if the race wants that.  Never blocks: finished event pairs
// are collected as they come.
static int pick(mcraw_ctx *c, Tuner::Entry &x, TuneTimer &tm)
{
    for (size_t i = 0; i < x.pending.size();) {
        if (hipEventQuery(x.pending[i].b) != hipSuccess) {
            (void)hipGetLastError(); // (hipErrorNotReady is no error)
            i++;
            continue;
        }
        float ms = 0.f;
        const bool read = hipEventElapsedTime(&ms, x.pending[i].a, x.pending[i].b) == hipSuccess;
        x.race.sample(x.pending[i].cand, read ? ms : 0.f);
        c->event_pool.insert(c->event_pool.end(), {x.pending[i].a, x.pending[i].b});
        x.pending.erase(x.pending.begin() + static_cast<long>(i));
    }
    tm.c = c, tm.e = &x, tm.cand = x.race.next();
    return tm.cand >= 0 ? tm.cand : x.race.current();
}

void TuneTimer::begin(hipStream_t st_)
{
    if (cand < 0)
        return;
    st = st_, a = get_event(c), b = get_event(c);
    if (a && b)
        (void)hipEventRecord(a, st);
}

void TuneTimer::end()
{
    if (cand < 0)
        return;
    if (a && b) {
        (void)hipEventRecord(b, st);
        e->pending.push_back({a, b, cand});
    } else { // (no events to be had, or the batch failed before its launch: the race hears that the sample is lost)
        for (hipEvent_t ev : {a, b})
            if (ev)
                c->event_pool.push_back(ev);
        e->race.sample(cand, 0.f);
    }
    cand = -1;
}

uint32_t tune_xcd(mcraw_ctx *c, int n7, uint32_t R, uint32_t mode, TuneTimer &tm)
{
    Tuner::Entry &x = entry_of(c, c->xcd, n7, R, mode);
    if (!x.race.nc) // runs of 128 workgroups, the grid in eight parts (submit())
        x.cand[0][0] = 128, x.cand[1][0] = 0, x.race.reset(2);
    return static_cast<uint32_t>(x.cand[pick(c, x, tm)][0]);
}

void tune_side(mcraw_ctx *c, int n7, uint32_t R, int nsplit[2], TuneTimer &tm)
{
    Tuner::Entry &x = entry_of(c, c->side, n7, R, 0u);
    if (!x.race.nc) {
        // (512 workgroups of k7_side are resident at once; parts that own little leave early, so somewhat more can pay:
        // 120 x 8K frames ran fastest with 4 + 1 parts = 600 workgroups, tools/side_split.py)
        const int budget = 1024 / std::max(n7, 1);
        static const int all[][2] = {{4, 4}, {4, 2}, {4, 1}, {2, 2}, {2, 4}, {3, 1}, {1, 3}, {1, 1}}; // (unsplit can win too)
        int nc = 0;
        for (const auto &cd : all)
            if (cd[0] + cd[1] <= budget && nc < Race::MAXC)
                x.cand[nc][0] = cd[0], x.cand[nc][1] = cd[1], nc++;
        if (nc == 0)
            x.cand[0][0] = x.cand[0][1] = 1, nc = 1;
        x.race.reset(nc);
    }
    const int *cd = x.cand[pick(c, x, tm)];
    nsplit[0] = cd[0], nsplit[1] = cd[1];
}

const int *tune_decided(const Tuner &t) { return t.last && t.last->race.decided >= 0 ? t.last->cand[t.last->race.decided] : nullptr; }

void tune_release(mcraw_ctx *c)
{
    for (KStat &k : c->kstat)
        for (; !k.pending.empty(); k.pending.pop_back())
            c->event_pool.insert(c->event_pool.end(), {k.pending.back().first, k.pending.back().second});
    for (Tuner *t : {&c->xcd, &c->side})
        for (Tuner::Entry &x : t->entries)
            for (; !x.pending.empty(); x.pending.pop_back())
                c->event_pool.insert(c->event_pool.end(), {x.pending.back().a, x.pending.back().b});
}

// ---- the host-memory pipeline's trials (HostWay)
// Status words home behind their kernels (1), or fetched at the wait (0)?  In a process whose first GPU work was this context
// sending is 10 % faster for a large batch (2 960 against 2 680 UHD frames/s); behind one torch operation -- HIP hands a process four
// hardware queues per stream priority, and which of the context's streams share one depends on what existed before -- the small
// kernel that writes home makes sub-batch k + 1's upload wait for sub-batch k's download there (1 600 against 2 570).  Neither a
// probe on dummy buffers nor the first pieces of a batch show that (it sets in later), so whole batches are compared: of the
// batches of ten pieces or more the first one fetches and only warms the slots up, the second fetches, the third and the fourth
// send (the fourth is the one compared), and the faster way is the context's for large batches from then on (until then:
// fetched).  Streams of short tickets decide for themselves (ticket_way: sending won wherever it was measured).
// MCRAW_SHORT_WAY=0|1 decides both beforehand.

void way_from_env(mcraw_ctx *c)
{
    HostWay &w = c->way;
    if (c->env_short_way >= 0 && w.send_home < 0)
        w.send_home = w.send_home_tickets = c->env_short_way;
    // (a context that shares its device does not compare -- the others' traffic is in its times --: it takes what a context of
    // this device found, if one has)
    if (w.send_home < 0 && !alone_on_device(c) && c->device >= 0 && c->device < 64) {
        std::lock_guard<std::mutex> lk(g_gate[c->device].mu);
        if (g_gate[c->device].way >= 0)
            w.send_home = w.send_home_tickets = g_gate[c->device].way;
    }
}

int host_way(const mcraw_ctx *c, bool tickets) { return tickets ? c->way.send_home_tickets : c->way.send_home; }

// The way of a batch of more than one piece; *trial: it is one of the two that are compared (big_way_result when it is over).
int big_way(mcraw_ctx *c, size_t total, bool *trial)
{
    HostWay &w = c->way;
    way_from_env(c);
    *trial = w.send_home < 0 && alone_on_device(c) && total / PIECE_BYTES >= 10;
    if (w.send_home >= 0)
        return w.send_home;
    if (*trial && w.big_seen++ == 0) {
        *trial = false; // (the context's first large batch pays for the slots' buffers: fetched, and not compared)
        // ... and what the other way needs is made now, so that its trial batch does not pay for it: the slots' pinned status
        // buffers, the first launch of the kernel that writes into them
        for (Slot &x : c->slots)
            if (ensure(x.status_host, 4096, true) != 0)
                break;
        if (c->slots[0].status_host.p) {
            warm_send_status(c->slots[0].stream);
            (void)hipStreamSynchronize(c->slots[0].stream);
        }
        (void)hipGetLastError();
    }
    return *trial && w.trial_rate[0] != 0.0 ? 1 : 0;
}

void big_way_result(mcraw_ctx *c, int way, size_t total, double seconds)
{
    HostWay &w = c->way;
    if (w.send_home >= 0 || seconds <= 0)
        return;
    if (way == 1 && w.sent_trials++ == 0)
        return; // (the first batch that sends is its way's warm-up, as the context's first batch was the other's)
    w.trial_rate[way] = total / seconds;
    if (way == 1) {
        w.send_home = w.trial_rate[1] > w.trial_rate[0] * 1.03 ? 1 : 0;
        if (c->device >= 0 && c->device < 64) {
            std::lock_guard<std::mutex> lk(g_gate[c->device].mu);
            g_gate[c->device].way = w.send_home;
        }
        if (c->env_trace)
            std::fprintf(stderr, "[mcraw] host-memory pipeline: status words fetched %.1f GB/s, sent home %.1f GB/s: %s from here on\n",
                         w.trial_rate[0] / 1e9, w.trial_rate[1] / 1e9, w.send_home ? "sent" : "fetched");
    }
}

// ... and for a caller that streams short tickets instead (the facade's chunks): TRIAL_TICKETS in a row fetch, the next
// TRIAL_TICKETS send, the rate between the first and the last landing of each row is compared.
constexpr int TRIAL_TICKETS = 12;

int ticket_way(mcraw_ctx *c, mcraw_ticket *t, int nframes, size_t total)
{
    HostWay &w = c->way;
    way_from_env(c);
    if (total > PIECE_BYTES) { // a large batch as a ticket: compared like the synchronous ones, its time runs until it is waited for
        t->way = big_way(c, total, &t->big_trial);
        t->trial_bytes = total;
        t->t_queued = std::chrono::steady_clock::now();
    } else if (w.send_home_tickets >= 0) {
        t->way = w.send_home_tickets;
    } else if (nframes > 0 && alone_on_device(c) && w.tt.queued < TRIAL_TICKETS) {
        t->way = t->trial_way = w.tt.way; // (undecided: this ticket belongs to the row under way)
        t->trial_bytes = total;
        w.tt.queued++;
    } // (else: fetched, as a ticket is made)
    return t->way;
}

void ticket_never_flew(mcraw_ctx *c, const mcraw_ticket *t)
{
    if (t->trial_way >= 0 && c->way.tt.queued > 0)
        c->way.tt.queued--; // (a ticket that never flew lands nowhere: its place in the trial row is free again)
}

void ticket_landed(mcraw_ctx *c, const mcraw_ticket *t, int rc)
{
    if (t->big_trial && rc == 0)
        big_way_result(c, t->way, t->trial_bytes, std::chrono::duration<double>(std::chrono::steady_clock::now() - t->t_queued).count());
    if (t->trial_way < 0 || c->way.send_home_tickets >= 0 || t->trial_way != c->way.tt.way)
        return;
    HostWay::TicketTrial &tt = c->way.tt; // a ticket of the trial row under way has landed
    const auto now = std::chrono::steady_clock::now();
    if (tt.landed++ == 0)
        tt.t_first = now; // (the row's clock starts with its first landing; that ticket's bytes are not counted)
    else
        tt.bytes += t->trial_bytes;
    if (tt.landed != TRIAL_TICKETS)
        return;
    tt.rate[tt.way] = tt.bytes / std::max(1e-9, std::chrono::duration<double>(now - tt.t_first).count());
    if (tt.way == 0) {
        tt = HostWay::TicketTrial{1, 0, 0, 0, now, {tt.rate[0], 0.0}};
    } else {
        c->way.send_home_tickets = tt.rate[1] > tt.rate[0] * 1.03 ? 1 : 0;
        if (c->env_trace)
            std::fprintf(stderr, "[mcraw] host-memory pipeline (tickets): status words fetched %.1f GB/s, sent home %.1f GB/s: %s from here on\n",
                         tt.rate[0] / 1e9, tt.rate[1] / 1e9, c->way.send_home_tickets ? "sent" : "fetched");
    }
}


} // namespace mcraw
