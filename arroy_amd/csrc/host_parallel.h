// host_parallel.h — the one host-thread helper of the library, in a header with no device include so that the host-only
// headers (forest_records.h) and their stand-alone checkers can use it.
#pragma once

#include <thread>
#include <vector>

namespace ah {

// fn(0) .. fn(n - 1), fn(0) on the calling thread and the others on threads of their own.  A thread that cannot be created
// (std::system_error) must not cross the C ABI: its share simply runs on the caller.
template <class F>
inline void parallel_run(unsigned n, F fn) {
    std::vector<std::thread> pool;
    unsigned started = 1;
    try {
        pool.reserve(n);
        for (; started < n; started++) pool.emplace_back(fn, started);
    } catch (...) {
    }
    if (n) fn(0u);
    for (unsigned t = started; t < n; t++) fn(t);
    for (auto &th : pool) th.join();
}

}  // namespace ah
