// Stand-alone driver of the dose record's part of rtd::FieldMemory (raytracedicom_amd/csrc/rtd_field_memory.hpp).
// tests/test_dose_record_memory.py builds it (also with -fsanitize=address,undefined) and runs it on the CPU.
//
// The dose record has no life of its own: it is allocated, recorded, usable and dropped with the sigma record. The driver walks two
// field memories in lock step over random sequences of events (fixed seed), driven as the engine drives them:
//   `with`     the field under test: the dose record allowed or not (RTD_NO_DOSE_REPLAY), its allocation failing or not, the sigma
//              record's allocation failing or not;
//   `without`  the same events with the dose record switched off.
// After every event:
//   - everything the sigma record decides and shows is the same on both sides (the dose record changes nothing about it);
//   - `without` never has a dose record; `with` has one exactly where the rule says: dose_reused is 0 or equals sigma_reused, the dose
//     record's extent is 0 or the sigma record's; while it is allowed and no allocation of it has failed, it is always the latter of
//     each; once its allocation has failed it is never asked for again and the sigma record goes on being replayed.
//
//   test_rtd_dose_record [walks per configuration] [events per walk]      (defaults 1500, 96)
// Exit code 1 at the first violation (with the walk, the event and the observable), 3 if the walk left an observable at one value.
// Prints one line "ok ..." with the counts.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "rtd_field_memory.hpp"

namespace {

struct Coverage {
    long events = 0, dose[3] = {}, sigmaWithoutDose = 0, doseAllocFailed = 0, notTriedAgain = 0, regrown = 0, releases = 0;
    bool complete() const { return dose[0] > 0 && dose[1] > 0 && dose[2] > 0 && sigmaWithoutDose > 0 && doseAllocFailed > 0 && notTriedAgain > 0 && regrown > 0 && releases > 0; }
};

#define CHECK(what, cond)                                                                                               \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            std::printf("violated: configuration %d walk %d event %d (%s): %s\n", cfg, w, e, name, what);               \
            return false;                                                                                               \
        }                                                                                                               \
    } while (0)

// The launch as rtd_field_compute_bev makes it: decide, launched, then the allocations (the sigma record's first; the dose record's
// only behind a sigma record that stands).
rtd::LaunchDecision launch(rtd::FieldMemory& m, unsigned epoch, bool capturing, bool noDose, bool sigmaAllocFails, bool doseAllocFails) {
    const rtd::LaunchDecision d = m.decide(rtd::LaunchInputs{epoch, capturing, true, false, false, noDose});
    m.launched(d);
    if (d.sigma == rtd::SigmaRecord::kAllocateThenRecord) {
        if (sigmaAllocFails) m.sigmaAllocationFailed();
        else if (d.dose && doseAllocFails) m.doseAllocationFailed();
    }
    return d;
}

bool walkAll(int walks, int events, Coverage& cov) {
    for (int cfg = 0; cfg < 8; ++cfg) {
        const bool noDose = cfg & 1, doseAllocFails = cfg & 2, sigmaAllocFails = cfg & 4;
        std::mt19937 rng(7100u + (unsigned)cfg);
        auto draw = [&](unsigned n) { return (unsigned)(rng() % n); };
        for (int w = 0; w < walks; ++w) {
            auto with = std::make_unique<rtd::FieldMemory>();             // (on the heap: the sanitizer watches both ends of it)
            auto without = std::make_unique<rtd::FieldMemory>();
            unsigned epoch = draw(3);
            bool computed = false, failedBefore = false;
            for (int e = 0; e < events; ++e) {
                const unsigned r = draw(100);
                const char* name = "";
                ++cov.events;
                if (r < 6) { name = "inputs changed"; ++epoch; }
                else if (r < 45) {
                    name = "launch";
                    const bool capturing = draw(8) == 0;
                    const size_t stepsBefore = with->doseSteps;
                    const rtd::LaunchDecision a = launch(*with, epoch, capturing, noDose, sigmaAllocFails, doseAllocFails);
                    const rtd::LaunchDecision b = launch(*without, epoch, capturing, true, sigmaAllocFails, false);
                    computed = true;
                    CHECK("the sigma record's decision", a.sigma == b.sigma && a.need == b.need && a.flight.reuse == b.flight.reuse);
                    CHECK("a dose record only with a sigma record", !a.dose || a.sigma != rtd::SigmaRecord::kWalk);
                    CHECK("no dose record when switched off", !b.dose && !(noDose && a.dose));
                    CHECK("never while capturing", !(capturing && (a.dose || a.flight.dose)));
                    if (a.sigma == rtd::SigmaRecord::kAllocateThenRecord && a.dose && stepsBefore > 0) ++cov.regrown;
                    if (failedBefore && a.sigma != rtd::SigmaRecord::kWalk) { CHECK("not tried again", !a.dose); ++cov.notTriedAgain; }
                    if (a.sigma == rtd::SigmaRecord::kAllocateThenRecord && a.dose && doseAllocFails && !sigmaAllocFails) { ++cov.doseAllocFailed; failedBefore = true; }
                    ++cov.dose[with->flight.dose];
                    if (with->flight.sigma && !with->flight.dose) ++cov.sigmaWithoutDose;
                } else if (r < 80) {
                    if (!computed) continue;
                    name = "finish";
                    const bool big = draw(2);
                    const rtd::FieldFindings fd{draw(5) == 0 ? 1 : 0, draw(6) == 0, false, draw(2) ? 8 : 20, big ? 5 : 10, big ? 125 : 50};
                    const bool va = with->finished(fd), vb = without->finished(fd);
                    CHECK("the verdict", va == vb);
                } else if (r < 88) {
                    if (!computed) continue;
                    name = "sigma record finished";
                    const int err = draw(5) == 0 ? 1 : 0;
                    with->sigmaFinished(err); without->sigmaFinished(err);
                } else if (r < 97) { name = "set spot weights"; with->forgetHints(); without->forgetHints(); }
                else {
                    name = "release";
                    ++cov.releases;
                    *with = rtd::FieldMemory{}; *without = rtd::FieldMemory{};
                    computed = false; failedBefore = false;
                }
                const int ds = computed ? with->flight.dose : 0, sg = computed ? with->flight.sigma : 0;
                CHECK("sigma_reused", sg == (computed ? without->flight.sigma : 0));
                CHECK("the sigma record's extent", with->sigmaSteps == without->sigmaSteps);
                CHECK("the sigma record's state", with->sigma.usable == without->sigma.usable && with->sigma.launched == without->sigma.launched &&
                                                  with->sigmaFailed == without->sigmaFailed);
                CHECK("dose_reused is 0 or sigma_reused", ds == 0 || ds == sg);
                CHECK("the dose record's extent is 0 or the sigma record's", with->doseSteps == 0 || with->doseSteps == with->sigmaSteps);
                CHECK("no dose record where it is switched off", without->doseSteps == 0 && without->flight.dose == 0 && !(noDose && (with->doseSteps || ds)));
                if (!noDose && !with->doseFailed) {
                    CHECK("the dose record goes with the sigma record", with->doseSteps == with->sigmaSteps && ds == sg);
                }
                if (with->doseFailed) CHECK("a failed dose record is gone", with->doseSteps == 0 && ds == 0);
            }
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const int walks = argc > 1 ? std::atoi(argv[1]) : 1500, events = argc > 2 ? std::atoi(argv[2]) : 96;
    if (walks <= 0 || events <= 0) { std::fprintf(stderr, "usage: %s [walks per configuration] [events per walk]\n", argv[0]); return 2; }
    Coverage cov;
    if (!walkAll(walks, events, cov)) return 1;
    if (!cov.complete()) { std::printf("the walk leaves an observable at one value\n"); return 3; }
    std::printf("ok events %ld dose walked %ld recorded %ld replayed %ld sigma_without_dose %ld dose_alloc_failed %ld then_not_tried_again %ld "
                "record_regrown %ld releases %ld\n", cov.events, cov.dose[0], cov.dose[1], cov.dose[2], cov.sigmaWithoutDose, cov.doseAllocFailed,
                cov.notTriedAgain, cov.regrown, cov.releases);
    return 0;
}
