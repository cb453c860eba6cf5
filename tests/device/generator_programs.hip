// k_generate_level<F, true> and k_generate_chain<F, true> (csrc/generators.hpp: the generator kernels with generator programs, the
// registers in dynamic LDS) on the GPU, built for gfx950 from the headers alone: the schedule that csrc/generator_schedule.hpp makes
// of a circuit with program generators is run on the device through gen::launch_generators and the values of every class come
// back.  Nothing is compared here: tests/test_device_generator_programs.py holds GeneratorProgram.evaluate.
//   generator_programs <in> <out>       (the word file of tests/sanitize/program_case.hpp, every case with input values)
// out: as tests/host_shim/generators.cpp writes it.  A schedule is checked (program_case::sound: every index inside its array,
// every program op inside the tables) before anything is launched.  Exit status 3: malformed file, 6: unsound schedule, 7: a HIP
// call failed.
#include <hip/hip_runtime.h>

#include "generators.hpp"
#include "program_case.hpp"

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
static int run(const program_case::Case& pc, const gen::Schedule& s, std::vector<uint64_t>* out) {
    typedef typename F::T T;
    const schedule_case::Case& c = pc.circuit;
    const size_t nc = s.num_classes, ni = s.input_cls.size();
    std::vector<T> in(ni);
    std::vector<u32> scatter(s.input_cls);
    for (size_t i = 0; i < ni; i++) {
        in[i] = (T)c.values[i];
        if (s.input_first[i] != i) scatter[i] = gen::OUT_SKIP;
    }
    std::vector<uint64_t> lits_host(pc.programs.lits.size());
    for (size_t i = 0; i < lits_host.size(); i++) lits_host[i] = (uint64_t)F::enc(pc.programs.lits[i]);
    gen::Op* ops = nullptr;
    gen::ProgramHeader* headers = nullptr;
    uint64_t *instrs = nullptr, *lits = nullptr, *row_constants = nullptr;
    u32 *args = nullptr, *level_off = nullptr, *cls = nullptr, *err = nullptr;
    T *in_dev = nullptr, *values = nullptr;
    HIP_OK(upload(s.ops, &ops));
    HIP_OK(upload(s.args, &args));
    HIP_OK(upload(s.level_off, &level_off));
    HIP_OK(upload(scatter, &cls));
    HIP_OK(upload(in, &in_dev));
    HIP_OK(upload(pc.programs.headers, &headers));
    HIP_OK(upload(pc.programs.instrs, &instrs));
    HIP_OK(upload(lits_host, &lits));
    HIP_OK(upload(s.row_constants, &row_constants));
    HIP_OK(hipMalloc((void**)&values, (nc ? nc : 1) * sizeof(T)));
    HIP_OK(hipMalloc((void**)&err, gen::ERROR_WORDS * sizeof(u32)));
    HIP_OK(hipMemset(values, 0, (nc ? nc : 1) * sizeof(T)));
    HIP_OK(hipMemset(err, 0, gen::ERROR_WORDS * sizeof(u32)));
    if (ni) hipLaunchKernelGGL(gen::k_scatter_inputs<F>, dim3((unsigned)((ni + gen::GROUP - 1) / gen::GROUP)), dim3(gen::GROUP), 0, 0, cls, in_dev, (u32)ni, values);
    gen::DeviceSchedule d{nullptr, nullptr, nullptr};
    std::string msg;
    if (!gen::device_schedule(s, ops, args, level_off, headers, instrs, lits, row_constants, &d, &msg)) return 6;
    gen::launch_generators<F>(d, s.launches.data(), s.launches.size(), s.level_off.data(), values, err, 0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<T> got(nc ? nc : 1);
    u32 err_host[gen::ERROR_WORDS];
    HIP_OK(hipMemcpy(got.data(), values, got.size() * sizeof(T), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(err_host, err, sizeof(err_host), hipMemcpyDeviceToHost));
    for (void* p : {(void*)ops, (void*)args, (void*)level_off, (void*)cls, (void*)err, (void*)in_dev, (void*)values, (void*)headers, (void*)instrs,
                    (void*)lits, (void*)row_constants})
        (void)hipFree(p);
    for (uint64_t v : {(uint64_t)s.num_classes, (uint64_t)s.num_levels, (uint64_t)s.launches.size(), (uint64_t)s.num_unrunnable}) out->push_back(v);
    out->insert(out->end(), s.class_reps.begin(), s.class_reps.end());
    for (size_t k = 0; k < nc; k++) out->push_back((uint64_t)got[k]);
    for (u32 e : err_host) out->push_back(e);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 3;
    std::vector<uint64_t> in, out;
    if (!schedule_case::read_words(argv[1], &in) || in.empty()) return 3;
    size_t pos = 1;
    for (uint64_t k = 0; k < in[0]; k++) {
        program_case::Case c;
        if (!program_case::parse(in, &pos, &c) || !c.circuit.has_values) return 3;
        gen::Schedule s;
        std::string msg;
        const int status = program_case::schedule(&c, &s, &msg);
        out.push_back((uint64_t)status);
        if (status) {
            std::printf("case %llu: %s\n", (unsigned long long)k, msg.c_str());
            continue;
        }
        if (!program_case::sound(c, s)) return 6;
        for (uint64_t v : c.circuit.values)
            if (v >= c.circuit.order) return 3;
        if (const int r = c.circuit.ext_degree == 2 ? run<GlF>(c, s, &out) : run<BbF>(c, s, &out)) return r;
    }
    if (pos != in.size()) return 3;
    return schedule_case::write_words(argv[2], out) ? 0 : 3;
}
