// sample_law_check -- the law the noise table must match, drawn the way the reference draws it (util/rlwe.cpp:57-99, restated):
// a double from std::normal_distribution(0, 3.2), drawn again while its magnitude exceeds 19.2, then truncated toward zero
// by the conversion to an integer. Prints the histogram of 2^20 such samples over std::mt19937 with a fixed seed, one
// "value count" line per signed value -19 .. 19, then the sampling rate. tests/test_sample_host.py compares the histogram
// with tests/golden/noise_cdt.json by chi-square.
//   sample_law_check [log2 of the sample count, default 20]
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

int main(int argc, char **argv)
{
    const int log_count = argc > 1 ? std::atoi(argv[1]) : 20;
    if (log_count < 0 || log_count > 30)
        return 2;
    const std::uint64_t count = std::uint64_t(1) << log_count;
    const double sigma = 3.2, max_deviation = 6 * sigma;
    std::mt19937 gen(20240607u);
    std::normal_distribution<double> normal(0.0, sigma);
    std::uint64_t hist[39] = { 0 };
    const auto t0 = std::chrono::steady_clock::now();
    for (std::uint64_t i = 0; i < count; i++)
    {
        double x;
        do
            x = normal(gen);
        while (std::fabs(x) > max_deviation);
        const std::int64_t v = static_cast<std::int64_t>(x); // truncates toward zero
        hist[v + 19]++;
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int v = -19; v <= 19; v++)
        std::printf("%d %llu\n", v, static_cast<unsigned long long>(hist[v + 19]));
    std::printf("samples_per_second %.0f\n", static_cast<double>(count) / seconds);
    return 0;
}
