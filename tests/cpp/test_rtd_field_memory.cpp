// Stand-alone driver of rtd::FieldMemory (raytracedicom_amd/csrc/rtd_field_memory.hpp): what a field keeps between computes.
// tests/test_field_memory_reference.py builds it (also with -fsanitize=address,undefined) and runs it on the CPU.
//
// `Old` below is a literal transcription, restricted to the flags, of the rules as the engine wrote them out by hand before the header
// existed: rtd_field_compute_bev, sigmaMode, the radius test of launchSuperposition, takeFindings, sigmaRecordFinished, and the writes
// of rtd_field_dose_influence, rtd_field_set_spot_weights and rtd_field_release (f-> and h-> dropped, hipMalloc replaced by a flag
// that says whether it fails). The driver walks `Old` and the header in lock step over random sequences of events (fixed seed) and
// compares every observable after every event.
//
// Events: the inputs change (epoch + 1); a launch, capturing or not; a finish with findings drawn from {error flag} x {empty} x
// {uniform} x {maxRadius 8, 20} x {two plan extents}, drawn anew at every finish (so a finish repeated for one launch, with the same
// or with other findings, and two launches before one finish all occur); the sigma record's "finished" on its own; new spot weights;
// hints saved, forgotten, restored; release. A released field object is deleted when its workspace is taken over: after comparing what
// a fetch would read the walk goes on with a fresh field on both sides. Finishes are drawn only while the field counts as computed
// (the engine refuses them otherwise, in front of these rules).
// Fixed per walk: trace reuse allowed, uniformEligible, noSigmaReuse, the record's allocation fails (16 configurations).
//
//   test_rtd_field_memory [walks per configuration] [events per walk]      (defaults 1500, 96: 16 x 1500 x 96 = 2 304 000 events)
// First the transcription alone: the walk must make every observable take every value (else exit code 3, nothing is compared). Then
// the lock step (first difference: exit code 1, with the walk, the event and the observable). Prints one line "ok ..." with the counts.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "rtd_field_memory.hpp"

namespace {

constexpr int kSwMaxR = 16;       // the reach of the sweep's first launch, as the engine passes it in

struct Findings { int errorFlags, empty, uniformField, maxRadius, beamFirstInside, firstGuaranteedPassive; };

// What one launch decides, as both sides report it. sigma: 0 walk, 1 allocate `need` steps then record, 2 record, 3 replay.
struct Launch { bool reuse, tryUniform, knownUniform, runBig, selfPlanned; int sigma; size_t need; int sigmaRole; };

// ---- the rules as they were written by hand ----------------------------------------------------------------------------------------
struct Old {
    int uniformHint = -1, radiusHint = -1;
    unsigned hintEpoch = 0, launchEpoch = 0;
    bool launchedKnownUniform = false, triedUniform = false;
    bool traceLaunched = false; unsigned traceEpoch = 0; bool traceUsable = false; bool launchedReuse = false;
    int planFirst = 0, planSteps = 0;
    size_t sigRecSteps = 0; bool sigRecFailed = false, sigRecLaunched = false; unsigned sigRecEpoch = 0; bool sigRecUsable = false;
    int launchedSigma = 0;
    bool selfPlanned = false;

    int sigmaDecision = 0; size_t sigmaNeed = 0;   // (the driver's: which way sigmaMode went)
    int sigmaMode(unsigned inputEpoch, bool reuse, bool noSigmaReuse, bool allocFails) {
        sigmaDecision = 0; sigmaNeed = 0;
        if (!reuse || noSigmaReuse || sigRecFailed) return 0;
        const size_t need = (size_t)std::max(planSteps, 1);
        if (sigRecSteps >= need && sigRecUsable && sigRecEpoch == inputEpoch) { sigmaDecision = 3; return 2; }
        sigmaDecision = 2;
        if (sigRecSteps < need) {
            sigmaDecision = 1; sigmaNeed = need;
            sigRecSteps = need;
            if (allocFails) {
                sigRecSteps = 0; sigRecFailed = true; sigRecLaunched = false; sigRecUsable = false;
                return 0;
            }
        }
        sigRecLaunched = true; sigRecEpoch = inputEpoch; sigRecUsable = false;
        return 1;
    }
    Launch launch(unsigned inputEpoch, bool capturing, bool allowed, bool uniformEligible, bool noSigmaReuse, bool allocFails) {
        bool reuse = traceUsable && traceEpoch == inputEpoch && allowed;
        if (capturing) reuse = false;
        if (!reuse) { traceUsable = false; traceLaunched = !capturing; traceEpoch = inputEpoch; }
        launchedReuse = reuse;
        const bool tryUniform = uniformEligible && !(uniformHint == 0 && hintEpoch == inputEpoch);
        triedUniform = tryUniform;
        launchEpoch = inputEpoch;
        const bool knownUniform = tryUniform && uniformHint == 1 && hintEpoch == inputEpoch;
        launchedKnownUniform = knownUniform;
        launchedSigma = sigmaMode(inputEpoch, reuse, noSigmaReuse, allocFails);
        // launchSuperposition (a field with the sweep, without the halo and without RTD_SEPARATE_KS_PLAN)
        const bool selfPlan = !tryUniform;
        selfPlanned = selfPlan;
        const bool radiusKnown = radiusHint >= 0 && hintEpoch == inputEpoch;
        const bool runSweep = !knownUniform;
        const bool runBig = runSweep && !(radiusKnown && radiusHint <= kSwMaxR);
        return Launch{reuse, tryUniform, knownUniform, runBig, selfPlan, sigmaDecision, sigmaNeed, launchedSigma};
    }
    void sigmaRecordFinished(int errorFlags) {
        if (errorFlags) { sigRecUsable = false; sigRecLaunched = false; return; }
        if (sigRecLaunched && sigRecEpoch == launchEpoch) sigRecUsable = true;
    }
    bool takeFindings(const Findings& st) {   // -> the RTD_ERR_NOT_READY verdict (remote: false, every caller refuses remote fields first)
        const bool remote = false;
        sigmaRecordFinished(st.errorFlags);
        if (!st.errorFlags && !remote) {
            planFirst = st.beamFirstInside;
            planSteps = st.empty ? 0 : std::max(st.firstGuaranteedPassive - st.beamFirstInside, 0);
        }
        if (triedUniform) { uniformHint = st.uniformField ? 1 : 0; hintEpoch = launchEpoch; }
        else if (hintEpoch != launchEpoch) { uniformHint = -1; hintEpoch = launchEpoch; }
        radiusHint = (st.errorFlags || st.empty) ? -1 : st.maxRadius;
        traceUsable = traceLaunched && launchEpoch == traceEpoch && !st.errorFlags && !remote;
        return launchedKnownUniform && !st.uniformField && !st.errorFlags && !st.empty;
    }
    void forgetHints() { uniformHint = -1; radiusHint = -1; }
    void release() {
        traceLaunched = false; traceUsable = false;
        sigRecSteps = 0; sigRecLaunched = false; sigRecUsable = false; launchedSigma = 0;
    }
};
struct OldHints { int uniform, radius; unsigned epoch; };

// ---- the header, driven as the engine drives it ------------------------------------------------------------------------------------
Launch launchNew(rtd::FieldMemory& m, unsigned epoch, bool capturing, bool allowed, bool uniformEligible, bool noSigmaReuse, bool allocFails) {
    const rtd::LaunchDecision d = m.decide(rtd::LaunchInputs{epoch, capturing, allowed, uniformEligible, noSigmaReuse});
    m.launched(d);
    if (d.sigma == rtd::SigmaRecord::kAllocateThenRecord && allocFails) m.sigmaAllocationFailed();
    const bool selfPlan = !m.flight.tryUniform;
    m.planInsideSweep(selfPlan);
    const bool runBig = !m.flight.knownUniform && !m.radiusWithin(kSwMaxR);
    const int way = d.sigma == rtd::SigmaRecord::kWalk ? 0 : d.sigma == rtd::SigmaRecord::kAllocateThenRecord ? 1 : d.sigma == rtd::SigmaRecord::kRecord ? 2 : 3;
    return Launch{m.flight.reuse, m.flight.tryUniform, m.flight.knownUniform, runBig, m.flight.planInSweep, way,
                  way == 1 ? d.need : (size_t)0, m.flight.sigma};
}

struct Coverage {
    long reuse[2] = {}, sigma[4] = {}, knownUniform[2] = {}, runBig[2] = {}, tryUniform[2] = {}, verdict[2] = {};
    long allocFailed = 0, notTriedAgain = 0, events = 0, releases = 0, regrown = 0;
    bool complete() const {
        bool ok = verdict[1] > 0 && allocFailed > 0 && notTriedAgain > 0 && regrown > 0;
        for (int i = 0; i < 2; ++i) ok = ok && reuse[i] > 0 && knownUniform[i] > 0 && runBig[i] > 0 && tryUniform[i] > 0;
        for (int i = 0; i < 4; ++i) ok = ok && sigma[i] > 0;
        return ok;
    }
    void print(const char* head) const {
        std::printf("%s events %ld reuse %ld/%ld sigma walk %ld allocate %ld record %ld replay %ld known_uniform %ld/%ld second_sweep %ld/%ld try_uniform %ld/%ld "
                    "not_uniform_verdicts %ld alloc_failed %ld then_not_tried_again %ld record_regrown %ld releases %ld\n", head, events, reuse[0], reuse[1],
                    sigma[0], sigma[1], sigma[2], sigma[3], knownUniform[0], knownUniform[1], runBig[0], runBig[1], tryUniform[0], tryUniform[1], verdict[1],
                    allocFailed, notTriedAgain, regrown, releases);
    }
};

#define SAME(what, a, b)                                                                                                        \
    do {                                                                                                                        \
        if ((long long)(a) != (long long)(b)) {                                                                                 \
            std::printf("differs: configuration %d walk %d event %d (%s): %s was %lld, is %lld\n", cfg, w, e, name, what,        \
                        (long long)(a), (long long)(b));                                                                        \
            return false;                                                                                                       \
        }                                                                                                                       \
    } while (0)

// One pass over every configuration. compare = false: the transcription alone.
bool walkAll(int walks, int events, bool compare, Coverage& cov) {
    for (int cfg = 0; cfg < 16; ++cfg) {
        const bool allowed = cfg & 1, eligible = cfg & 2, noSigma = cfg & 4, allocFails = cfg & 8;
        std::mt19937 rng(20240u + (unsigned)cfg);
        auto draw = [&](unsigned n) { return (unsigned)(rng() % n); };
        for (int w = 0; w < walks; ++w) {
            auto old = std::make_unique<Old>();
            auto mem = std::make_unique<rtd::FieldMemory>();            // (on the heap: the sanitizer watches both ends of it)
            OldHints oldSaved{-1, -1, 0}; rtd::FieldHints newSaved;
            unsigned epoch = draw(3);                                    // (a field may be created after the handle's inputs changed)
            bool computed = false, failedBefore = false;
            for (int e = 0; e < events; ++e) {
                const unsigned r = draw(100);
                const char* name = "";
                ++cov.events;
                if (r < 6) { name = "inputs changed"; ++epoch; }
                else if (r < 40) {
                    name = "launch";
                    const bool capturing = draw(8) == 0;
                    const size_t stepsBefore = old->sigRecSteps;
                    const Launch a = old->launch(epoch, capturing, allowed, eligible, noSigma, allocFails);
                    computed = true;
                    ++cov.reuse[a.reuse]; ++cov.sigma[a.sigma]; ++cov.knownUniform[a.knownUniform]; ++cov.runBig[a.runBig]; ++cov.tryUniform[a.tryUniform];
                    if (a.sigma == 1 && stepsBefore > 0) ++cov.regrown;
                    if (failedBefore && a.reuse && !noSigma && a.sigma == 0) ++cov.notTriedAgain;
                    if (a.sigma == 1 && allocFails) { ++cov.allocFailed; failedBefore = true; }
                    if (compare) {
                        const Launch b = launchNew(*mem, epoch, capturing, allowed, eligible, noSigma, allocFails);
                        SAME("reuse", a.reuse, b.reuse); SAME("tryUniform", a.tryUniform, b.tryUniform); SAME("knownUniform", a.knownUniform, b.knownUniform);
                        SAME("second sweep launch", a.runBig, b.runBig); SAME("selfPlanned", a.selfPlanned, b.selfPlanned);
                        SAME("sigma decision", a.sigma, b.sigma); SAME("need", a.need, b.need); SAME("sigma role", a.sigmaRole, b.sigmaRole);
                    }
                } else if (r < 72) {
                    if (!computed) continue;
                    name = "finish";
                    const bool big = draw(2);
                    const Findings fd{draw(5) == 0 ? 1 : 0, draw(6) == 0 ? 1 : 0, (int)draw(2), draw(2) ? 8 : 20, big ? 5 : 10, big ? 125 : 50};
                    const bool a = old->takeFindings(fd);
                    ++cov.verdict[a];
                    if (compare) {
                        const bool b = mem->finished(rtd::FieldFindings{fd.errorFlags, fd.empty != 0, fd.uniformField != 0, fd.maxRadius, fd.beamFirstInside,
                                                                        fd.firstGuaranteedPassive});
                        SAME("not-uniform verdict", a, b);
                    }
                } else if (r < 80) {
                    if (!computed) continue;
                    name = "sigma record finished";
                    const int err = draw(5) == 0 ? 1 : 0;
                    old->sigmaRecordFinished(err);
                    if (compare) mem->sigmaFinished(err);
                } else if (r < 86) { name = "set spot weights"; old->forgetHints(); if (compare) mem->forgetHints(); }
                else if (r < 89) { name = "hints saved"; oldSaved = OldHints{old->uniformHint, old->radiusHint, old->hintEpoch}; if (compare) newSaved = mem->savedHints(); }
                else if (r < 94) { name = "hints forgotten"; old->forgetHints(); if (compare) mem->forgetHints(); }
                else if (r < 97) {
                    name = "hints restored";
                    old->uniformHint = oldSaved.uniform; old->radiusHint = oldSaved.radius; old->hintEpoch = oldSaved.epoch;
                    if (compare) mem->restoreHints(newSaved);
                } else {
                    name = "release";
                    ++cov.releases;
                    old->release(); computed = false;
                    if (compare) *mem = rtd::FieldMemory{};
                }
                if (compare) {   // what the engine reads between events (of a released field: a fetch and the buffer table only)
                    SAME("trace_reused", computed && old->launchedReuse, computed && mem->flight.reuse);
                    SAME("sigma_reused", computed ? old->launchedSigma : 0, computed ? mem->flight.sigma : 0);
                    SAME("record extent", old->sigRecSteps, mem->sigmaSteps);
                    if (r < 97) {
                        SAME("planSteps", old->planSteps, mem->planSteps); SAME("planFirst", old->planFirst, mem->planFirst);
                        SAME("selfPlanned", old->selfPlanned, mem->flight.planInSweep);
                    }
                }
                if (r >= 97) {   // (the released object is deleted at the takeover: a fresh field on both sides)
                    old = std::make_unique<Old>(); mem = std::make_unique<rtd::FieldMemory>();
                    oldSaved = OldHints{-1, -1, 0}; newSaved = rtd::FieldHints{}; failedBefore = false;
                }
            }
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const int walks = argc > 1 ? std::atoi(argv[1]) : 1500, events = argc > 2 ? std::atoi(argv[2]) : 96;
    if (walks <= 0 || events <= 0) { std::fprintf(stderr, "usage: %s [walks per configuration] [events per walk]\n", argv[0]); return 2; }
    Coverage alone;
    walkAll(walks, events, false, alone);
    alone.print("transcription");
    if (!alone.complete()) { std::printf("the walk leaves an observable at one value: nothing compared\n"); return 3; }
    Coverage both;
    if (!walkAll(walks, events, true, both)) return 1;
    if (!both.complete() || both.events != alone.events) { std::printf("the lock step walked other events than the transcription alone\n"); return 3; }
    both.print("ok");
    return 0;
}
