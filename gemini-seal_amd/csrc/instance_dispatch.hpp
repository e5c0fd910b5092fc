// instance_dispatch.hpp -- from a run-time value to the template instance compiled for it. A launcher whose kernel family
// is instantiated over a range (ND = 1..16) or a set ({30, 31}, {4, 8, 16, 32, 64}) hands the value and a generic lambda
// to one of these; the lambda gets the value as a std::integral_constant and launches `kernel<decltype(v)::value>`. The
// result says whether an instance matched: the launcher's fallback (loop kernel, generic instance, refusal) is its `else`.
// The range is written once, as the template arguments -- which instances exist is what the call instantiates.
// No HIP: tests/mac_select_check.cpp compiles this header with a host compiler.
#pragma once
#include <type_traits>
#include <utility>

namespace sealhip
{
    // f(std::integral_constant<int, V>{}) for the V among Vs... equal to value; false: none was
    template <int... Vs, class F>
    bool dispatch_among(int value, F &&f)
    {
        return ((value == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
    }

    namespace detail
    {
        template <int Lo, class F, int... Is>
        bool dispatch_from(int value, F &&f, std::integer_sequence<int, Is...>)
        {
            return dispatch_among<(Lo + Is)...>(value, f);
        }
    } // namespace detail

    // the same over every V in [Lo, Hi]
    template <int Lo, int Hi, class F>
    bool dispatch_int(int value, F &&f)
    {
        static_assert(Lo <= Hi, "an empty range has no instance");
        return detail::dispatch_from<Lo>(value, f, std::make_integer_sequence<int, Hi - Lo + 1>{});
    }

    // f(std::true_type{}) or f(std::false_type{}): both instances exist, nothing to fall back to
    template <class F>
    void dispatch_bool(bool value, F &&f)
    {
        if (value)
            f(std::true_type{});
        else
            f(std::false_type{});
    }
} // namespace sealhip
