// rtd_field_memory.hpp — what a field learns from its computes and keeps for the next ones, and the decisions taken from it. Host
// only: plain C++17, no HIP, no kernel constant; a device never sees any of it (tests/cpp/test_rtd_field_memory.cpp compiles it alone
// and walks it in lock step with the rules as they were once written out by hand in the engine). DESIGN.md section 4, "What a field
// keeps between computes", states the rule; this file is the rule.
//
// Everything here is valid for the INPUTS it was learned under: the handle counts every change of CT, LUTs or options (its input
// epoch), and whatever was launched under one epoch is used under that epoch only. The engine calls, in this order,
//   decide()    before a compute's launches: which of them are left out          (rtd_field_compute_bev)
//   launched()  once the compute is certain to be launched as decided
//   finished()  whenever the state record of the launched compute is known on the host (rtd_field_wait_plan, rtd_field_finish, ...)
// and nothing but this file writes the state.
#pragma once
#include <algorithm>
#include <cstddef>

namespace rtd {

// Something a compute leaves on the device that later computes can use instead of making it again (the trace with the plan; the
// sigma record). It is LAUNCHED under an epoch, becomes USABLE once a compute launched under that epoch has been seen finished
// without a device error flag, and is used only while the handle's epoch is still that one.
// kErrorForgetsLaunch: a finish that saw an error flag also forgets that anything was launched, so that a later clean finish of the
// same launch does not make it usable. The two users differ in this (DESIGN.md names the one sequence on which it shows).
template <bool kErrorForgetsLaunch>
struct KeptUnderEpoch {
    bool launched = false, usable = false;
    unsigned epoch = 0;
    // leavesRecord = false: a launch into a capturing stream runs when its graph does, not now
    void launch(unsigned underEpoch, bool leavesRecord = true) { usable = false; launched = leavesRecord; epoch = underEpoch; }
    bool usableUnder(unsigned handleEpoch) const { return usable && epoch == handleEpoch; }
    // the compute launched under launchEpoch (the last one launched) is known to be finished; ok: without a device error flag
    void finished(unsigned launchEpoch, bool ok) {
        usable = ok && launched && epoch == launchEpoch;
        if (!ok && kErrorForgetsLaunch) launched = false;
    }
    void drop() { launched = false; usable = false; }
};

// What the last finished compute found, under the epoch it was launched under. With a ray-weight cut-off above 0 both move with the
// spot weights: rtd_field_set_spot_weights forgets them.
struct FieldHints {
    int uniform = -1;             // 0 heterogeneous, 1 one sigma per slice, -1 unknown
    int radius = -1;              // largest batch radius (-1 unknown)
    unsigned epoch = 0;
    bool knownHeterogeneous(unsigned e) const { return uniform == 0 && epoch == e; }
    bool knownUniform(unsigned e) const { return uniform == 1 && epoch == e; }
    bool radiusWithin(unsigned e, int maxR) const { return radius >= 0 && epoch == e && radius <= maxR; }
    void forget() { uniform = -1; radius = -1; }
};

// The compute in flight: what its launch was decided to be (the last launched compute, finished or not).
struct ComputeInFlight {
    unsigned epoch = 0;           // the handle's epoch at the launch: what its findings are valid for
    bool reuse = false;           // neither tracer nor scan nor plan were launched (rtd_field_fetch "trace_reused")
    bool tryUniform = false;      // the uniform-sigma detection ran
    bool knownUniform = false;    // the general superposition kernel was left out on the strength of the hint
    int sigma = 0;                // k_fill's sigma role: 0 walked, 1 recorded and replayed, 2 replayed (rtd_field_fetch "sigma_reused")
    bool planInSweep = false;     // no k_ks_plan launch: block 0 of k_superpose_sweep's launch was the plan
    int dose = 0;                 // k_fill's dose role, likewise (rtd_field_fetch "dose_reused"): never ahead of `sigma`
};

// What a launch is decided from, besides the memory.
struct LaunchInputs {
    unsigned epoch;               // the handle's
    bool capturing;               // the stream is capturing: nothing is reused, and the launch leaves no record
    bool traceReuseAllowed;       // the field's configuration lets a compute go without tracer, scan and plan at all
    bool uniformEligible;         // the separable superposition may take the field
    bool noSigmaReuse;            // RTD_NO_SIGMA_REUSE
    bool noDoseReplay = false;    // RTD_NO_DOSE_REPLAY
};

enum class SigmaRecord { kWalk, kAllocateThenRecord, kRecord, kReplay };   // no record / make room for `need` steps first / record / replay

struct LaunchDecision {
    ComputeInFlight flight;       // (planInSweep: set by the superposition's launch, planInsideSweep)
    bool capturing;
    SigmaRecord sigma;
    size_t need;                  // kAllocateThenRecord: the step extent to allocate
    bool dose = false;            // the dose record goes with the sigma record: allocated, recorded or replayed as `sigma` says
};

// What a finished compute's state record tells the host.
struct FieldFindings {
    int errorFlags;
    bool empty, uniformField;
    int maxRadius, beamFirstInside, firstGuaranteedPassive;
};

struct FieldMemory {
    FieldHints hints;
    ComputeInFlight flight;
    KeptUnderEpoch<false> trace;  // density, WEPL, radiation length, entry / exit steps, WEPL minima, the plan's part of the records
    KeptUnderEpoch<true> sigma;   // the sigma record (rtd_fill.hpp), kept under the trace's rule
    int planFirst = 0, planSteps = 0;   // beamFirstInside and the steps up to firstGuaranteedPassive of the trace in use
    size_t sigmaSteps = 0;        // extent of the sigma record's step axis (0: no record allocated)
    bool sigmaFailed = false;     // its allocation failed once: not tried again
    // The dose record (rtd_fill.hpp) shares the sigma record's life: allocated with it at the same extent, recorded by the same pass,
    // usable under the same epoch, dropped by the same events. It has no state of its own but whether it exists beside the sigma record.
    size_t doseSteps = 0;         // extent of the dose record's step axis: sigmaSteps, or 0 (no dose record: the dose role walks)
    bool doseFailed = false;      // its allocation alone failed once: the field replays sigma and walks the dose, not tried again

    // The launch of a compute under `in`, decided and not yet recorded (the caller may still fail in front of its first launch).
    LaunchDecision decide(const LaunchInputs& in) const {
        LaunchDecision d{};
        d.capturing = in.capturing;
        ComputeInFlight& c = d.flight;
        c.epoch = in.epoch;
        c.planInSweep = flight.planInSweep;
        // the trace and the plan of a finished compute stand while CT, LUTs and options do; a graph must not depend on what the field
        // knew when it was captured
        c.reuse = trace.usableUnder(in.epoch) && in.traceReuseAllowed && !in.capturing;
        // the detection and the uniform kernel are left out for a field found heterogeneous under the same inputs; a field found
        // uniform under them will be found uniform again (the test is exact arithmetic on the same values)
        c.tryUniform = in.uniformEligible && !hints.knownHeterogeneous(in.epoch);
        c.knownUniform = c.tryUniform && hints.knownUniform(in.epoch);
        d.sigma = SigmaRecord::kWalk;
        if (c.reuse && !in.noSigmaReuse && !sigmaFailed) {
            d.need = (size_t)std::max(planSteps, 1);
            if (sigmaSteps < d.need) d.sigma = SigmaRecord::kAllocateThenRecord;
            else d.sigma = sigma.usableUnder(in.epoch) ? SigmaRecord::kReplay : SigmaRecord::kRecord;
        }
        c.sigma = d.sigma == SigmaRecord::kWalk ? 0 : (d.sigma == SigmaRecord::kReplay ? 2 : 1);
        // (a record allocated anew gets its dose record with it; one that stands has it or not)
        d.dose = d.sigma != SigmaRecord::kWalk && !in.noDoseReplay && !doseFailed &&
                 (d.sigma == SigmaRecord::kAllocateThenRecord || doseSteps == sigmaSteps);
        c.dose = d.dose ? c.sigma : 0;
        return d;
    }
    // The compute is launched as decided. (kAllocateThenRecord: the caller allocates next, and reports a failure.)
    void launched(const LaunchDecision& d) {
        flight = d.flight;
        if (!d.flight.reuse) trace.launch(d.flight.epoch, !d.capturing);
        if (d.sigma == SigmaRecord::kAllocateThenRecord) { sigmaSteps = d.need; doseSteps = d.dose ? d.need : 0; }
        if (d.sigma == SigmaRecord::kAllocateThenRecord || d.sigma == SigmaRecord::kRecord) sigma.launch(d.flight.epoch);
    }
    // The allocation asked for failed: no error, the compute in flight and every later one walk the recurrence.
    void sigmaAllocationFailed() { sigmaSteps = 0; sigmaFailed = true; sigma.drop(); flight.sigma = 0; doseSteps = 0; flight.dose = 0; }
    // The dose record's allocation alone failed: no error, the sigma record stands, the dose role of this and every later compute walks.
    void doseAllocationFailed() { doseSteps = 0; doseFailed = true; flight.dose = 0; }
    void planInsideSweep(bool inSweep) { flight.planInSweep = inSweep; }
    // The sweep's second launch (batch radius beyond maxR) can be left out of the compute in flight.
    bool radiusWithin(int maxR) const { return hints.radiusWithin(flight.epoch, maxR); }

    // A compute launched behind the sigma record's pass is known to be finished (a batch of rtd_field_dose_influence has drained).
    void sigmaFinished(int errorFlags) { sigma.finished(flight.epoch, errorFlags == 0); }
    // The state record of the compute in flight is on the host. The hints belong to the inputs the compute was LAUNCHED under: CT, LUTs
    // or options may have changed since. -> true: the compute was launched as a uniform-sigma field and is not one (it skipped the
    // general kernel and has written no BEV dose: the caller changed a bound device volume in place without telling the handle).
    bool finished(const FieldFindings& fd) {
        const bool ok = fd.errorFlags == 0;
        sigmaFinished(fd.errorFlags);
        if (ok) {                 // (what the scan and the plan found: the same for every compute that reuses them)
            planFirst = fd.beamFirstInside;
            planSteps = fd.empty ? 0 : std::max(fd.firstGuaranteedPassive - fd.beamFirstInside, 0);
        }
        if (flight.tryUniform) { hints.uniform = fd.uniformField ? 1 : 0; hints.epoch = flight.epoch; }
        else if (hints.epoch != flight.epoch) { hints.uniform = -1; hints.epoch = flight.epoch; }
        hints.radius = (!ok || fd.empty) ? -1 : fd.maxRadius;
        trace.finished(flight.epoch, ok);   // (a later compute may run on another stream: usable only once seen finished)
        return flight.knownUniform && !fd.uniformField && ok && !fd.empty;
    }

    // rtd_field_set_spot_weights and the batches of rtd_field_dose_influence, which saves the hints in front of them and puts them back
    void forgetHints() { hints.forget(); }
    FieldHints savedHints() const { return hints; }
    void restoreHints(const FieldHints& saved) { hints = saved; }
};

}  // namespace rtd
