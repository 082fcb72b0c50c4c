// Event detection for the batch integrator.
//
// Reference: include/heyoka/events.hpp (t_event_batch / nt_event_batch), src/detail/event_detection.cpp
// (ed_data_batch<T>::detect_events(), :1733-2173), src/taylor_adaptive_batch.cpp:727-1030 (the event branch of
// step_impl()). The reference detects events on the host, one batch lane after the other, with JIT-compiled
// helpers for the polynomial translations. Here the detection runs on the device, one lane per system:
// fast exclusion check (interval Horner enclosure), Collins-Akritas root isolation with Descartes' rule on
// the translated polynomials, bracketed root finding, direction filter and terminal-event cooldowns; the
// (few) detected events are then copied to the host, which runs the reference's sequential logic (ordering,
// step truncation at the first terminal event, callbacks, cooldown bookkeeping, outcomes).
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <optional>
#include <ostream>
#include <string>
#include <utility>
#include <vector>

#include "event_action.hpp"
#include "expression.hpp"
#include "kernel_args.hpp"

namespace heyoka_amd
{

enum class event_direction : int { negative = -1, any = 0, positive = 1 };

// (src/nt_event.cpp:42-54.)
inline std::ostream &operator<<(std::ostream &os, event_direction dir)
{
    switch (dir) {
        case event_direction::any:
            return os << "event_direction::any";
        case event_direction::positive:
            return os << "event_direction::positive";
        case event_direction::negative:
            return os << "event_direction::negative";
    }
    return os << "event_direction::??";
}

namespace detail
{

// Type-erased events as stored in the integrator core. ctx is the address of the user-facing integrator object
// (taylor_adaptive_batch<double> *, or the C handle), supplied at call time.
struct core_nt_event {
    expression eq;
    std::function<void(void *ctx, double time, int d_sgn, std::uint32_t batch_idx)> callback;
    event_direction dir = event_direction::any;
    // (See core_t_event::native_counter: hy_event_counter_nt.)
    std::uint64_t *native_counter = nullptr;
    // (See core_t_event::recorder: hy_event_recorder_nt.)
    bool recorder = false;
};

struct core_t_event {
    expression eq;
    std::function<bool(void *ctx, int d_sgn, std::uint32_t batch_idx)> callback; // empty -> always stop
    event_direction dir = event_direction::any;
    double cooldown = -1; // < 0: deduced automatically (taylor_deduce_cooldown())
    // The callback is the library's own counting callback (hy_event_counter_t of the C ABI: increments *counter and lets
    // the integration continue): nothing of the caller's runs, so the step applies it on the device.
    std::uint64_t *native_counter = nullptr;
    // The callback is the library's recording callback (hy_event_recorder_t of the C ABI, the tag event_recorder of the
    // C++ interface): every invocation appends a row to the integrator's event log (see event_log_header) and lets the
    // integration continue; native_counter, if set, is incremented as by the counting callback.
    bool recorder = false;
    // The callback is a library-side action (event_action.hpp): assignments to state variables applied by the
    // kernel hy_ev_action, on the device when every event of the integrator is library-side, in a one-system launch at
    // the callback's place in the host loop otherwise. It continues; `callback` is not invoked.
    std::shared_ptr<const event_action> action;
};

// One detected event of a lane: (event index, root (time from the beginning of the step), sign of the time
// derivative of the event equation, absolute value of the derivative).
struct detected_event {
    std::uint32_t idx;
    double root;
    int d_sgn;
    double abs_der;
};

// Capacity of the per-lane list of detected events of one class (terminal / non-terminal) in a step: every event
// equation is a polynomial of degree `order` over the step, so (order + 1) entries per event of the class hold
// whatever a successful root isolation can produce (the reference's lists are unbounded vectors).
std::uint32_t ed_max_detected(std::uint32_t order, std::uint32_t n_te, std::uint32_t n_nte);

// Limit on the working list of the root isolation: the reference's (src/detail/event_detection.cpp:1399, :2082).
inline constexpr std::uint32_t ed_work_list_cap = 250;
// Bytes of working list per resident thread ("slot") of hy_detect_events.
std::size_t ed_work_list_bytes_per_slot(std::uint32_t order);

// HIP source of the detection kernel for a given Taylor order and list capacity.
std::string make_event_detection_source(std::uint32_t order, std::uint32_t max_detected);

// ---- event log (library-side recording callbacks, core_*_event::recorder) ----
// A row of the log: event_log_header doubles (system, class - 0 terminal / 1 non-terminal -, event index within the
// class, d_sgn, trigger time hi, trigger time lo, root, |d eq/dt| at the root), then - unless the states are switched
// off - the dim state variables at the trigger time.
inline constexpr std::uint32_t event_log_header = 8;

// HIP source of the kernels which turn the detected events of one step into the row headers of the log, in the order in
// which the host loop would have invoked the callbacks: hy_evr_count (rows per lane + sums per workgroup of 256 lanes),
// hy_evr_scan (one workgroup: exclusive scan of the workgroup sums, in as many passes of 256 as it takes), hy_evr_write
// (in-workgroup scan, sort of the lane's events, headers). A module of its own: the event-detection module of an
// integrator without recorders is not touched.
std::string make_event_recorder_source(std::uint32_t max_detected);

} // namespace detail

} // namespace heyoka_amd
