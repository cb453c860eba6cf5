// k_scatter_inputs, k_generate_level<F>, k_generate_chain<F> and k_gather_public (csrc/generators.hpp) on the GPU, built for
// gfx950 from the headers alone: the schedule that csrc/generator_schedule.hpp makes of a described circuit is run on the device
// and the values of every class come back.  Nothing is compared here: tests/test_device_generators.py holds the builder mirror's
// generators.
//   generators <in> <out> plan|level     (the word file of tests/sanitize/schedule_case.hpp, every case with input values)
// plan: the schedule's own launches (chain kernel for runs of narrow levels); level: every level through k_generate_level.
// out: as tests/host_shim/generators.cpp writes it, the error word and `num_public_inputs` gathered values after each case's values.
// A schedule is checked (schedule_case::sound: every index inside its array) before anything is launched.  Exit status 3:
// malformed file, 6: unsound schedule, 7: a HIP call failed.
#include <hip/hip_runtime.h>

#include <cstring>

#include "generators.hpp"
#include "schedule_case.hpp"

using namespace gbk;

#define HIP_OK(expr)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));              \
            return 7;                                                                    \
        }                                                                                \
    } while (0)

template <class T>
static hipError_t upload(const std::vector<T>& host, T** dev) {
    hipError_t e = hipMalloc((void**)dev, host.size() ? host.size() * sizeof(T) : 16);
    if (e == hipSuccess && !host.empty()) e = hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

template <class F>
static int run(const schedule_case::Case& c, const gen::Schedule& s, bool level_kernel_only, std::vector<uint64_t>* out) {
    typedef typename F::T T;
    const size_t nc = s.num_classes, ni = s.input_cls.size(), npi = s.pi_cls.size();
    std::vector<T> in(ni);
    std::vector<u32> scatter(s.input_cls);
    for (size_t i = 0; i < ni; i++) {
        in[i] = (T)c.values[i];
        if (s.input_first[i] != i) scatter[i] = gen::OUT_SKIP;
    }
    gen::Op* ops = nullptr;
    u32 *args = nullptr, *level_off = nullptr, *cls = nullptr, *pi_cls = nullptr, *err = nullptr;
    T *in_dev = nullptr, *values = nullptr;
    u64* back = nullptr;
    HIP_OK(upload(s.ops, &ops));
    HIP_OK(upload(s.args, &args));
    HIP_OK(upload(s.level_off, &level_off));
    HIP_OK(upload(scatter, &cls));
    HIP_OK(upload(s.pi_cls, &pi_cls));
    HIP_OK(upload(in, &in_dev));
    HIP_OK(hipMalloc((void**)&values, (nc ? nc : 1) * sizeof(T)));
    HIP_OK(hipMalloc((void**)&err, gen::ERROR_WORDS * sizeof(u32)));
    HIP_OK(hipMalloc((void**)&back, (npi + gen::ERROR_WORDS) * sizeof(u64)));
    HIP_OK(hipMemset(values, 0, (nc ? nc : 1) * sizeof(T)));
    HIP_OK(hipMemset(err, 0, gen::ERROR_WORDS * sizeof(u32)));
    if (ni) hipLaunchKernelGGL(gen::k_scatter_inputs<F>, dim3((unsigned)((ni + gen::GROUP - 1) / gen::GROUP)), dim3(gen::GROUP), 0, 0, cls, in_dev, (u32)ni, values);
    if (level_kernel_only) {
        for (u32 l = 0; l < s.num_levels; l++) {
            const u32 first = s.level_off[l], count = s.level_off[l + 1] - first;
            if (count) hipLaunchKernelGGL(gen::k_generate_level<F>, dim3((count + gen::GROUP - 1) / gen::GROUP), dim3(gen::GROUP), 0, 0, ops, args, first, count, values, err);
        }
    } else {
        const gen::DeviceSchedule d{ops, args, level_off};
        gen::launch_generators<F>(d, s.launches.data(), s.launches.size(), s.level_off.data(), values, err, 0);
    }
    const u32 threads = npi > gen::ERROR_WORDS ? (u32)npi : gen::ERROR_WORDS;
    hipLaunchKernelGGL(gen::k_gather_public<F>, dim3((threads + gen::GROUP - 1) / gen::GROUP), dim3(gen::GROUP), 0, 0, pi_cls, (u32)npi, values, err, back);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<T> got(nc ? nc : 1);
    std::vector<u64> gathered(npi + gen::ERROR_WORDS);
    HIP_OK(hipMemcpy(got.data(), values, got.size() * sizeof(T), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(gathered.data(), back, gathered.size() * sizeof(u64), hipMemcpyDeviceToHost));
    for (void* p : {(void*)ops, (void*)args, (void*)level_off, (void*)cls, (void*)pi_cls, (void*)err, (void*)in_dev, (void*)values, (void*)back}) (void)hipFree(p);
    for (uint64_t v : {(uint64_t)s.num_classes, (uint64_t)s.num_levels, (uint64_t)s.launches.size(), (uint64_t)s.num_unrunnable}) out->push_back(v);
    out->insert(out->end(), s.class_reps.begin(), s.class_reps.end());
    for (size_t k = 0; k < nc; k++) out->push_back((uint64_t)got[k]);
    for (size_t k = 0; k < gen::ERROR_WORDS; k++) out->push_back(gathered[npi + k]);
    for (size_t k = 0; k < npi; k++) out->push_back(gathered[k]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) return 3;
    const bool level_only = !std::strcmp(argv[3], "level");
    if (!level_only && std::strcmp(argv[3], "plan")) return 3;
    std::vector<uint64_t> in, out;
    if (!schedule_case::read_words(argv[1], &in) || in.empty()) return 3;
    size_t pos = 1;
    for (uint64_t k = 0; k < in[0]; k++) {
        schedule_case::Case c;
        if (!schedule_case::parse(in, &pos, &c) || !c.has_values) return 3;
        gen::Schedule s;
        std::string msg;
        const int status = schedule_case::schedule(&c, &s, &msg);
        out.push_back((uint64_t)status);
        if (status) {
            std::printf("case %llu: %s\n", (unsigned long long)k, msg.c_str());
            continue;
        }
        if (!schedule_case::sound(c, s)) return 6;
        for (uint64_t v : c.values)
            if (v >= c.order) return 3;
        if (const int r = c.ext_degree == 2 ? run<GlF>(c, s, level_only, &out) : run<BbF>(c, s, level_only, &out)) return r;
    }
    if (pos != in.size()) return 3;
    return schedule_case::write_words(argv[2], out) ? 0 : 3;
}
