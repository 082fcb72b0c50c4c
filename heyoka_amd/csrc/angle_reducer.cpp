// callback::angle_reducer. See angle_reducer.hpp.
#include "angle_reducer.hpp"

#include <algorithm>
#include <ostream>
#include <set>
#include <stdexcept>
#include <string>

namespace heyoka_amd
{

namespace callback
{

struct angle_reducer::data {
    std::set<std::string> names;
    std::vector<std::size_t> positions;
};

namespace
{

[[noreturn]] void throw_unusable()
{
    throw std::invalid_argument("Cannot use an angle_reducer which was default-constructed or moved-from");
}

} // namespace

angle_reducer::angle_reducer() noexcept {}
angle_reducer::~angle_reducer() = default;

angle_reducer::angle_reducer(from_expressions, const std::vector<expression> &exs)
{
    if (exs.empty()) {
        throw std::invalid_argument("The list of expressions passed to the constructor of angle_reducer cannot be empty");
    }
    auto d = std::make_unique<data>();
    for (const auto &ex : exs) {
        if (!ex.is_variable()) {
            throw std::invalid_argument(
                "The list of expressions passed to the constructor of angle_reducer can contain only variables");
        }
        d->names.insert(ex.var_name());
    }
    m_data = std::move(d);
}

angle_reducer::angle_reducer(const angle_reducer &src)
{
    if (src.m_data) {
        m_data = std::make_unique<data>(*src.m_data);
    }
}

angle_reducer::angle_reducer(angle_reducer &&src) noexcept : m_data(std::move(src.m_data)) {}

angle_reducer &angle_reducer::operator=(const angle_reducer &src)
{
    // (Copy first: a throwing copy leaves the target as it was, and self-assignment needs no special case.)
    std::unique_ptr<data> fresh;
    if (src.m_data) {
        fresh = std::make_unique<data>(*src.m_data);
    }
    m_data.swap(fresh);
    return *this;
}

angle_reducer &angle_reducer::operator=(angle_reducer &&src) noexcept
{
    if (this != &src) {
        m_data = std::move(src.m_data);
    }
    return *this;
}

void angle_reducer::pre_hook(detail::tab_core &core)
{
    if (!m_data) {
        throw_unusable();
    }
    auto &ind = m_data->positions;
    ind.clear();
    const auto &sys = core.get_sys();
    for (std::size_t i = 0; i < sys.size(); ++i) {
        const auto &ex = sys[i].first;
        if (ex.is_variable() && m_data->names.count(ex.var_name()) != 0u) {
            ind.push_back(i);
        }
    }
}

bool angle_reducer::operator()(detail::tab_core &core)
{
    if (!m_data) {
        throw_unusable();
    }
    const auto &ind = m_data->positions;
    const auto n_sv = core.get_sys().size();
    if (!ind.empty() && ind.back() >= n_sv) {
        throw std::invalid_argument("Inconsistent state detected in angle_reducer: the last index in the indices vector has a "
                                    "value of "
                                    + std::to_string(ind.back()) + ", but the number of state variables is only "
                                    + std::to_string(n_sv));
    }
    core.angle_reduce(std::vector<std::uint32_t>(ind.begin(), ind.end()));
    return true;
}

void angle_reducer::pre_hook(taylor_adaptive_batch<double> &ta)
{
    pre_hook(ta.core());
}

bool angle_reducer::operator()(taylor_adaptive_batch<double> &ta)
{
    return (*this)(ta.core());
}

bool angle_reducer::is_valid() const noexcept
{
    return m_data != nullptr;
}

const std::vector<std::size_t> &angle_reducer::get_indices() const
{
    if (!m_data) {
        throw_unusable();
    }
    return m_data->positions;
}

// (The reference prints its unordered set of variables, "Angle reducer: {x, y}", in hash order: here sorted by name.)
std::ostream &operator<<(std::ostream &os, const angle_reducer &ar)
{
    if (!ar.m_data) {
        return os << "Angle reducer (default constructed)";
    }
    os << "Angle reducer: {";
    bool first = true;
    for (const auto &n : ar.m_data->names) {
        os << (first ? "" : ", ") << n;
        first = false;
    }
    return os << '}';
}

} // namespace callback

namespace detail
{

tab_core::red_t angle_reducer_indices_of(step_callback_batch<double> &cb)
{
    using ar_t = callback::angle_reducer;
    std::vector<ar_t *> members;
    if (auto *p = cb.extract<ar_t>()) {
        members.push_back(p);
    } else if (auto *set = cb.extract<step_callback_batch_set<double>>()) {
        for (std::size_t i = 0; i < set->size(); ++i) {
            auto *q = (*set)[i].extract<ar_t>();
            if (q == nullptr) {
                return {};
            }
            members.push_back(q);
        }
    }
    if (members.empty()) {
        return {};
    }
    // NOTE: the pointers refer to the objects stored in the callback, which the caller keeps alive for the whole call.
    return [members]() {
        std::set<std::uint32_t> u;
        for (const auto *m : members) {
            for (const auto i : m->get_indices()) {
                u.insert(static_cast<std::uint32_t>(i));
            }
        }
        return std::vector<std::uint32_t>(u.begin(), u.end());
    };
}

} // namespace detail

} // namespace heyoka_amd
