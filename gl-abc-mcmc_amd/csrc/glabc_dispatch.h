// glabc_dispatch.h -- run-time integer -> template parameter, for every launcher of the library (host only, no HIP).
//
//     return dispatch_range<1, 8>(dim, GLABC_ERR_DIM, [&](auto d) { return launch<decltype(d)::value>(args); });
//
// calls f(std::integral_constant<int, V>) for the one V of the set that equals v and returns f's int; a v outside the set
// returns `not_found` and calls nothing.  Exactly the listed V are instantiated.
#pragma once

#include <type_traits>
#include <utility>

namespace glabc {

template <int... Vs, class F>
int dispatch_values(int v, int not_found, F&& f)
{
    int rc = not_found;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}

template <int Lo, int... Is, class F>
int dispatch_offsets(int v, int not_found, F&& f, std::integer_sequence<int, Is...>)
{
    return dispatch_values<(Lo + Is)...>(v, not_found, f);
}

// the contiguous set Lo, Lo + 1, ..., Hi
template <int Lo, int Hi, class F>
int dispatch_range(int v, int not_found, F&& f)
{
    return dispatch_offsets<Lo>(v, not_found, f, std::make_integer_sequence<int, Hi - Lo + 1>{});
}

// two run-time integers of the same range at once: f(integral_constant<int, A>, integral_constant<int, B>)
template <int Lo, int Hi, class F>
int dispatch_pair(int a, int b, int not_found, F&& f)
{
    return dispatch_range<Lo, Hi>(a, not_found, [&](auto A) { return dispatch_range<Lo, Hi>(b, not_found, [&](auto B) { return f(A, B); }); });
}

}  // namespace glabc
