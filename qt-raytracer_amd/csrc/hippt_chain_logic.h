// hippt_chain_logic.h — the integer rules of chained batches (hippt_trace.h "chained batches",
// DESIGN.md §7) as pure functions: which batches a launch combines and traces, what its waves learn
// from the host mailbox, and the frame offset a wave traces a batch with; and, in the last section,
// the host's side of a run: when a batch continues it, when a batch is held, grouped or posted, what
// each launch, the mailbox and the final flush are told.  The gfx950 kernels call the device's rules
// and hippt_api.cpp (chain_batch, launch_held, flush_chain) the host's; tests/native/chain_model.cpp
// compiles this header with g++ and drives both through adversarial host/device interleavings
// (tests/test_chain_protocol.py), so its schedules vouch for the code that ships on either side.
//
// The anchor is the reference's frame-ordered accumulation: one launch and one sync per frame,
// every frame's sample blended into the running average in frame order
// (CudaPathTracerKernel.cu:157-178, 246-265).  A chained batch must therefore be traced exactly
// once, with the frames the host gave it, and combined exactly once, after every earlier batch.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HIPPT_CL __host__ __device__ __forceinline__
#else
#define HIPPT_CL inline
#endif

namespace hippt {
namespace chain {

// ---- the host mailbox word (pinned, coherent; host_add's word, stored by chain_batch) -----------
// run << 33 | consecutive frames << 32 | last posted batch
HIPPT_CL unsigned long long box_word(unsigned run, bool consecutive, unsigned last) {
    return ((unsigned long long)run << 33) | ((unsigned long long)(consecutive ? 1u : 0u) << 32) | last;
}

// ---- a block's view of the mailbox (LDS ChainView: last, flags) ---------------------------------
// kConsec: batch t + 1 renders the frames after batch t's (else the same frames again);
// kClosed: the host is on a later run (no batch after `last` will be posted);
// kStepKnown: kConsec is meaningful.  The host knows the run's frame pattern from its second batch
// on (chain_batch: seq 1 sets the step), so a view that knows any batch >= 1 is posted knows it.
constexpr unsigned kConsec = 1u, kClosed = 2u, kStepKnown = 4u;

// The view a launch starts with: batches up to `posted` (chainPosted) posted, its step chainStep
// (-1: not known when the launch was enqueued, which happens only for a run's batch 0).
HIPPT_CL unsigned view_flags_at_start(int step) {
    return step < 0 ? 0u : (kStepKnown | (step > 0 ? kConsec : 0u));
}

// The per-XCD device copy of the mailbox word: refresh stamp (16-tick units) << 40 | launch epoch
// mod 64 << 34 | closed << 33 | (an open run's) consecutive << 32 | last posted batch.  A host word
// of another run makes the copy "closed" and carries nothing else: the word's batch and frame
// pattern are the later run's.
HIPPT_CL unsigned long long copy_pack(unsigned long long now, unsigned long long h, unsigned run, unsigned ep) {
    const bool closed = unsigned(h >> 33) != run;
    return ((now >> 4) << 40) | ((unsigned long long)(ep & 63u) << 34) |
           (closed ? (1ull << 33) : (h & ((1ull << 33) - 1ull)));
}
HIPPT_CL bool copy_closed(unsigned long long c) { return ((c >> 33) & 1ull) != 0ull; }
HIPPT_CL unsigned copy_last(unsigned long long c) { return unsigned(c); }

// Merges a copy into a view.  Monotone: `last` never decreases and no flag is ever cleared, so a
// wave that reads the view's two words at any moment sees a pair some merge produced or a later
// `flags` beside an earlier `last`, and both say only true things.  A closed copy adds kClosed and
// nothing else; an open copy that knows a batch >= 1 is posted carries the run's frame pattern.
// (Round 5 replaced `flags` by the copy's: a closed copy then cleared kConsec while `last` kept a
// posted batch, and a wave that moved into that batch traced it with frame offset 0 — the
// GPUTEST_r05 failure, tests/native/chain_model.cpp legacy_view_merge.)
HIPPT_CL void view_merge(unsigned &last, unsigned &flags, unsigned long long c) {
    if (copy_closed(c)) {
        flags |= kClosed;
        return;
    }
    const unsigned cl = copy_last(c);
    if (cl > last) last = cl;
    if (cl >= 1u) flags |= kStepKnown | unsigned((c >> 32) & 1ull);
}

// chain_next's answer for batch nt from a view: posted (and the run's step known) or not.  A view
// that does not know the step never lets a wave take a batch: that batch's own launch traces it.
HIPPT_CL bool view_takes(unsigned nt, unsigned last, unsigned flags, int frames, int &step) {
    if (nt > last || !(flags & kStepKnown)) return false;
    step = (flags & kConsec) ? frames : 0;
    return true;
}

// ---- a launch's plan at its start (chain_begin) ------------------------------------------------
// Ring-slot marker of the last launch that moved into a slot's batch: batch << 32 | epoch + 1.
HIPPT_CL unsigned long long marker(unsigned t, unsigned epoch) { return ((unsigned long long)t << 32) | (epoch + 1u); }
// Batch t finished by a launch before this one (epoch e): an earlier launch took it, and every
// earlier launch has ended before this one started.
HIPPT_CL bool marker_finished(unsigned long long m, unsigned t, unsigned e) {
    const unsigned by = unsigned(m);
    return unsigned(m >> 32) == t && by != 0u && by <= e;
}
// Lane k of chain_begin's ballot looks at batch t0 + k when it is inside the ring's window.
HIPPT_CL bool begin_lane_in_window(unsigned k, unsigned t0, unsigned c0, unsigned slots) {
    return k < slots && t0 + k < c0 + slots;
}

struct BeginPlan {
    unsigned t0;    // the first batch whose marker the launch reads
    int c1;         // the launch combines [c0, c1] (none when c1 < c0)
    unsigned u;     // the first batch it traces
    unsigned tLim;  // the last batch it may trace
};
// c0: the first batch not combined by an earlier launch; own: chainSeq; nfin: the marked batches
// from t0 on (the run of finished batches the ballot found); slots: the ring; cap: chainCap.
HIPPT_CL unsigned begin_t0(unsigned c0, unsigned own) { return own > c0 ? own : c0; }
HIPPT_CL BeginPlan begin_plan(unsigned c0, unsigned own, unsigned nfin, unsigned slots, unsigned cap) {
    BeginPlan b;
    b.t0 = begin_t0(c0, own);
    const int a = int(b.t0 + nfin) - 1, o = int(own) - 1;
    b.c1 = a > o ? a : o;  // every batch before the own one, and the marked run from t0
    const int u = int(c0) > b.c1 + 1 ? int(c0) : b.c1 + 1;
    b.u = unsigned(u);
    const unsigned ringEnd = c0 + slots - 1u, capEnd = b.u + cap - 1u;
    b.tLim = ringEnd < capEnd ? ringEnd : capEnd;
    return b;
}
// The first batch not combined once this launch's combines are done (written for the next launch).
HIPPT_CL unsigned begin_next_c0(unsigned c0, int c1) { return int(c0) > c1 + 1 ? c0 : unsigned(c1 + 1); }

// ---- a wave moving on (chain_next) -------------------------------------------------------------
// The batch after the wave's batch t (the own group, ChainWave::stat, is followed by the batch after
// the group).
HIPPT_CL unsigned next_batch(unsigned t, unsigned stat, unsigned group) { return t == stat ? t + group : t + 1u; }
// The frames of batch tItem from the launch's own batch's (chainSeq): its step times the distance.
HIPPT_CL unsigned frame_add(unsigned tItem, unsigned own, int step) {
    return (tItem - own) * unsigned(step > 0 ? step : 0);
}
// The group position -> (batch, one-batch position) split of a group launch's queues: 64-item block
// m >> 6 is block (m >> 6) / group of batch t + (m >> 6) % group.
HIPPT_CL void group_item(unsigned got, unsigned t, unsigned group, unsigned &raw, unsigned &tItem) {
    if (group <= 1u) {
        raw = got;
        tItem = t;
        return;
    }
    const unsigned blk = got >> 6, q = blk / group;
    raw = (q << 6) | (got & 63u);
    tItem = t + (blk - q * group);
}

// ---- the host's side of a run -------------------------------------------------------------------
// What the host decides about a run, as a state machine over integers: whether a batch continues it
// (host_continues), a new run (host_open), what becomes of a batch (host_add: held for a group
// launch, launched with the held ones as one group, or posted in the mailbox and launched alone),
// the held group launched before a host-side wait (host_launch_held), and the final flush
// (host_close).  hippt_api.cpp (chain_batch, launch_held, flush_chain) does the HIP work around
// these calls and takes every number of a launch, of the mailbox and of the flush from their
// results; the model's host calls them in its schedules.  (The ring's slots for a cap:
// hippt_plan.h plan::ring_slots.)
struct HostRun {
    bool live = false;   // a run is open
    unsigned run = 0;    // its id
    unsigned seq = 0;    // the next batch's number in the run
    unsigned epoch = 0;  // the next launch's number in the run
    int firstFrame = 0;  // batch 0's first frame
    int step = -1;       // frames from one batch to the next (-1: one batch so far)
    unsigned cap = 0, slots = 0;
    // batches held for one group launch: their count and the first one's number (the group's own batch)
    unsigned pendN = 0, pendSeq = 0;
};

// A launch's chain fields: chainSeq, chainGroup, chainPosted, chainEpoch.
struct HostLaunch {
    unsigned own = 0, group = 1, posted = 0, epoch = 0;
};

// same: the caller's verdict that everything but the frames is the run's (the launch parameters, the
// grid, the geometry).  The run's second batch fixes its frame pattern: every batch the same frames
// (step 0), or the next ones (step = frames); later batches follow it or do not continue the run.
HIPPT_CL bool host_continues(HostRun &r, bool same, int firstFrame, int frames) {
    if (!r.live || !same) return false;
    if (r.seq == 1u) {
        const int d = firstFrame - r.firstFrame;
        if (d != 0 && d != frames) return false;
        r.step = d;
        return true;
    }
    return firstFrame == r.firstFrame + int(r.seq) * r.step;
}

// A new run (the old one closed first: host_close), of batches from firstFrame on.
HIPPT_CL void host_open(HostRun &r, int firstFrame, unsigned cap, unsigned slots) {
    r.live = true;
    r.run = (r.run + 1u) & 0x7fffffffu;
    r.seq = r.epoch = r.pendN = r.pendSeq = 0u;
    r.firstFrame = firstFrame;
    r.step = -1;
    r.cap = cap;
    r.slots = slots;
}

HIPPT_CL HostLaunch host_take_launch(HostRun &r, unsigned own, unsigned group, unsigned posted) {
    HostLaunch l;
    l.own = own, l.group = group, l.posted = posted, l.epoch = r.epoch++;
    r.pendN = 0u;
    return l;
}

// Which answers about the run's last enqueued launch host_add reads for the next batch — the one
// place that says so: host_add goes by it, and a caller asks the device for no more (the library: one
// hipEventQuery per answer; an answer that is not read may be anything).  A batch can only be held
// behind an earlier launch of the run, while the group has room, so otherwise neither is read.
// groupable: the caller allows groups for this batch (the library: its build knob, and 64-item runs
// only, since the group interleaves its batches' runs).  holdRunning: the batches that arrive while
// the run's only launch so far still runs are held too — the burst's second batch then opens the
// first group instead of being taken by that launch on its own walk of the item order and leaving
// its own launch nothing but the combine.
constexpr unsigned kReadsStarted = 1u;  // `started`
constexpr unsigned kReadsEnded = 2u;    // `ended`, where `started` is true
HIPPT_CL unsigned host_add_reads(const HostRun &r, bool groupable, bool holdRunning) {
    if (!(groupable && r.epoch > 0u && r.pendN + 1u < r.cap)) return 0u;
    return kReadsStarted | (holdRunning && r.epoch == 1u ? kReadsEnded : 0u);
}

enum HostAddKind { kAddHeld, kAddGroup, kAddAlone };
struct HostAdd {
    HostAddKind kind = kAddHeld;
    unsigned seq = 0;      // the batch's number in the run
    unsigned held = 0;     // batches held before this one
    HostLaunch launch;     // kAddGroup, kAddAlone: the launch to enqueue (kAddHeld: epoch = the next launch's)
    unsigned long long word = 0;  // kAddAlone: the mailbox word to store before the launch is enqueued
};
// The next batch of the open run.  started, ended: the run's last enqueued launch has started / has
// ended on the device (host_add_reads: which of them are read).  Held while
// that launch has not started and the group is not full; a batch that is not held is launched with
// the held ones as one group (own: the first held batch; none of them was posted, so no launch but
// the group's takes them), or posted and launched on its own.
HIPPT_CL HostAdd host_add(HostRun &r, bool groupable, bool started, bool ended, bool holdRunning) {
    HostAdd a;
    a.seq = r.seq++;
    a.held = r.pendN;
    a.launch.epoch = r.epoch;
    const unsigned reads = host_add_reads(r, groupable, holdRunning);
    if ((reads & kReadsStarted) && (!started || ((reads & kReadsEnded) && !ended))) {
        if (!r.pendN) r.pendSeq = a.seq;
        ++r.pendN;
        return a;
    }
    if (r.pendN) {
        a.kind = kAddGroup;
        a.launch = host_take_launch(r, r.pendSeq, r.pendN + 1u, a.seq);
        return a;
    }
    a.kind = kAddAlone;
    a.word = box_word(r.run, r.step > 0, a.seq);
    a.launch = host_take_launch(r, a.seq, 1u, a.seq);
    return a;
}

// The held batches launched now as one group, the run staying open: false when there are none.
HIPPT_CL bool host_has_held(const HostRun &r) { return r.live && r.pendN != 0u; }
HIPPT_CL bool host_launch_held(HostRun &r, HostLaunch &l) {
    if (!host_has_held(r)) return false;
    l = host_take_launch(r, r.pendSeq, r.pendN, r.seq - 1u);
    return true;
}

// The run's end: the held group's launch, if any, and then the final flush's fields (the run's
// launches were epochs 0 .. epoch - 1; it combines up to lastSeq).
struct HostClose {
    bool held = false;  // `launch` is to be enqueued before the flush
    HostLaunch launch;
    unsigned epoch = 0, lastSeq = 0;
    int step = 0;
};
HIPPT_CL bool host_close(HostRun &r, HostClose &c) {  // false: no run is open
    if (!r.live) return false;
    c.held = host_launch_held(r, c.launch);
    r.live = false;
    c.epoch = r.epoch;
    c.lastSeq = r.seq - 1u;
    c.step = r.step > 0 ? r.step : 0;
    return true;
}

}  // namespace chain
}  // namespace hippt
