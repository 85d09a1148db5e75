// dvbs2_rx_bb -- the RX graphs of the reference wired with the HIP modules (host/dvbs2hip_modules.hpp), fed from raw IQ
// files in the reference's Radio_user_binary format (native-endian interleaved re/im float32:
// src/common/Module/Radio/Radio_user_binary/Radio_user_binary.cpp:55-100).
//
//  (1) the RX half of dvbs2_tx_rx_bb (src/mains/TX_RX_BB/main.cpp:83-94), 2 * pl_frame values per frame:
//   dvbs2_rx_bb --mod-cod QPSK-S_8/9 -F 8 --dec-implem NMS --dec-ite 10 --in pl_frames.f32 --out info_bits.i32 [--src sent_bits.i32] [--frame-sync]
//      --frame-sync puts Synchronizer_frame_hip::synchronize in front, as src/mains/RX/main.cpp does; the input may then start
//      anywhere in a frame.  The SAME batch runs twice -- task by task through the sockets of the reference graph, and through
//      the fused Receiver_BB_hip task -- and the program fails if they differ.
//
//  (2) --matched-filter: the dvbs2_rx graph from the matched filter to the monitor (src/mains/RX/main_sched.cpp:199-223,
//      probes :244-247), 2 * pl_frame * osf values per frame (osf = 2 samples per symbol):
//   dvbs2_rx_bb --matched-filter --mod-cod QPSK-S_8/9 -F 4 --in shaped_stream.f32 --src sent_bits.i32 --src-delay 1 --mon-skip 1 --out info_bits.i32
//      The binding lines between the modules built here are the reference's, character for character (marked "main_sched.cpp:NNN").
//      The sample-serial loops in between are out of scope and are played by stand-ins defined below:
//      sync_coarse_f = identity (no frequency offset), sync_timing = decimation by osf at the even phase (perfect timing) unless
//      --stm-type FAST (or ULTRA [--stm-hold-size H] [--stm-learn-frames N]: the held loop, holding after N frames) binds Synchronizer_timing_hip (the Gardner loop, main_sched.cpp:202-204; a batch whose extract underflows stops
//      behind it, as the reference's sequence does at processing_aborted, and the payload source only advances for batches that go through); the source is a file of the sent payloads delayed by --src-delay frames (the frame synchronizer's latency;
//      what Filter_buffered_delay does in the TX_RX mains).
//      --wl-phases (with --stm-type FAST) runs the reference's waiting and learning phases on the head of the file first (main_sched.cpp:407-635): Synchronizer_step_mf_hip,
//      the coarse-frequency loop on the GPU, bound as main_sched.cpp:428-432 with a Feedbacker for DEL; --wl-frames L1 L2 L3 (150 150 200), --wl-wait-max (2000);
//      --smf-kernel LANE | WAVE chooses the loop's kernel (Synchronizer_step_mf_hip::set_kernel; not given: the library's default) and is refused without --wl-phases.
//
// With --src the monitor runs (check_errors in (1), check_errors2 with its BE / FE / BER / FER sockets read by probe stand-ins
// in (2)) and FRA / BE / FE are printed like the reference's terminal.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include "dvbs2hip_modules.hpp"

using namespace aff3ct;

// ---- stand-ins for StreamPU / dvbs2 modules that are outside the hot path: just enough surface for the binding lines
namespace spu { namespace module {
namespace src { enum class tsk : size_t { generate }; namespace sck { enum class generate : size_t { out_data, status }; } }
namespace prb { enum class tsk : size_t { probe }; namespace sck { enum class probe : size_t { in, status }; } }
class Source_file : public Module {          // Source_user_binary: payloads from a file, delayed by `delay` frames
public:
    Source_file(int K, int n_frames_, const std::string &path, int delay) : K(K), in(path, std::ios::binary), fifo((size_t)delay * K, 0)
    {
        if (!in) throw tools::runtime_error(__FILE__, __LINE__, __func__, "cannot open " + path);
        n_frames = (size_t)n_frames_;
        auto &t = create_task("generate");
        auto so = create_socket_out<int>(t, "out_data", K);
        create_codelet(t, [so](Module &m, runtime::Task &tk, size_t) -> int {
            auto &s = static_cast<Source_file &>(m);
            int *o = tk[so].get_dataptr<int>();
            const size_t n = (size_t)s.K * s.n_frames;
            std::vector<int> fresh(n, 0);
            s.in.read(reinterpret_cast<char *>(fresh.data()), n * sizeof(int));
            s.fifo.insert(s.fifo.end(), fresh.begin(), fresh.end());
            std::copy(s.fifo.begin(), s.fifo.begin() + n, o);
            s.fifo.erase(s.fifo.begin(), s.fifo.begin() + n);
            return 0;
        });
    }
    runtime::Socket &operator[](src::sck::generate s) { return (*tasks[0])[(size_t)s]; }
    runtime::Task &operator[](src::tsk) { return *tasks[0]; }
private:
    int K; std::ifstream in; std::vector<int> fifo;
};
// Feedbacker (StreamPU): `produce` hands out what `memorize` took at the iteration before (zeros at first) -- main_sched.cpp:429-430
namespace fbr { enum class tsk : size_t { produce, memorize }; namespace sck { enum class produce : size_t { Y_N, status }; enum class memorize : size_t { X_N, status }; } }
template <typename T> class Feedbacker : public Module {
public:
    Feedbacker(int size, T init, int n_frames_) : mem((size_t)size * n_frames_, init)
    {
        n_frames = (size_t)n_frames_;
        auto &p = create_task("produce");
        auto so = create_socket_out<T>(p, "Y_N", size);
        create_codelet(p, [so](Module &m, runtime::Task &tk, size_t) -> int {
            auto &f = static_cast<Feedbacker &>(m);
            std::copy(f.mem.begin(), f.mem.end(), tk[so].template get_dataptr<T>());
            return 0;
        });
        auto &q = create_task("memorize");
        auto si = create_socket_in<T>(q, "X_N", size);
        create_codelet(q, [si](Module &m, runtime::Task &tk, size_t) -> int {
            auto &f = static_cast<Feedbacker &>(m);
            const T *x = tk[si].template get_dataptr<const T>();
            std::copy(x, x + f.mem.size(), f.mem.begin());
            return 0;
        });
    }
    runtime::Socket &operator[](fbr::sck::produce s) { return (*tasks[0])[(size_t)s]; }
    runtime::Socket &operator[](fbr::sck::memorize s) { return (*tasks[1])[(size_t)s]; }
    runtime::Task &operator[](fbr::tsk t) { return *tasks[(size_t)t]; }
private:
    std::vector<T> mem;
};
template <typename T> class Probe_value : public Module {     // keeps the last value of the socket it is bound to
public:
    Probe_value(int size, const std::string &col, int n_frames_) : col(col)
    {
        n_frames = (size_t)n_frames_;
        auto &t = create_task("probe");
        auto si = create_socket_in<T>(t, "in", size);
        create_codelet(t, [si](Module &m, runtime::Task &tk, size_t) -> int {
            auto &p = static_cast<Probe_value &>(m);
            p.last = tk[si].template get_dataptr<const T>()[p.n_frames - 1];
            return 0;
        });
    }
    runtime::Socket &operator[](prb::sck::probe s) { return (*tasks[0])[(size_t)s]; }
    runtime::Task &operator[](prb::tsk) { return *tasks[0]; }
    T last = T();
    std::string col;
};
}}  // namespace spu::module
namespace aff3ct { namespace module {
class Sync_timing_perfect : public spu::module::Module {        // stand-in for Synchronizer_timing (Gardner, out of scope): even phase of osf = 2
public:
    Sync_timing_perfect(int N_in, int osf, int n_frames_)
    {
        n_frames = (size_t)n_frames_;
        auto &t = create_task("extract");
        auto sx = create_socket_in<float>(t, "X_N1", N_in);
        auto sy = create_socket_out<float>(t, "Y_N2", N_in / osf);
        create_codelet(t, [sx, sy, osf](spu::module::Module &, spu::runtime::Task &tk, size_t) -> int {
            const float *x = tk[sx].get_dataptr<const float>();
            float *y = tk[sy].get_dataptr<float>();
            const size_t n = tk[sy].get_n_elmts() / 2;
            for (size_t i = 0; i < n; i++) { y[2 * i] = x[2 * i * osf]; y[2 * i + 1] = x[2 * i * osf + 1]; }
            return 0;
        });
    }
    spu::runtime::Socket &in() { return (*tasks[0])[0]; }
    spu::runtime::Socket &out() { return (*tasks[0])[1]; }
    spu::runtime::Task &operator()() { return *tasks[0]; }
};
}}  // namespace aff3ct::module

static int run_matched_filter_graph(const std::string &modcod, int F, int n_ite, float alpha, const std::string &implem, const std::string &in_path,
                                    const std::string &out_path, const std::string &src_path, int src_delay, int mon_skip, float coarse_freq, bool stm_fast,
                                    bool wl_phases = false, int wl1 = 150, int wl2 = 150, int wl3 = 200, int wl_wait_max = 2000, bool stm_ultra = false, int stm_hold_size = 101,
                                    int stm_learn_frames = 500, int smf_kernel = -1)
{
    using namespace module;
    const int osf = 2;
    auto ctx = std::make_shared<Context>(modcod, F, n_ite, alpha, true, 0, implem);
    const int N_pl = 2 * ctx->sz.pl_frame_sym;
    std::vector<float> rx_samples((size_t)F * N_pl * osf);                       // what Radio::receive hands over
    // modules: unique_ptr + the reference's variable names, so that the binding lines below are the reference's own
    std::unique_ptr<Multiplier_AGC_hip>          front_agc    (new Multiplier_AGC_hip(ctx, N_pl * osf, 1.f / (float)osf));                // DVBS2.cpp:660-664 (build_channel_agc)
    std::unique_ptr<Multiplier_AGC_hip>          mult_agc     (new Multiplier_AGC_hip(ctx, N_pl, 1.f));                                  // DVBS2.cpp:653-657 (build_agc_shift)
    std::unique_ptr<Synchronizer_freq_coarse_hip<>> sync_coarse_f(new Synchronizer_freq_coarse_hip<>(ctx, N_pl * osf));                  // the frequency shift of the transmission phase
    sync_coarse_f->set_curr_freq(coarse_freq);                                                                                          // (what the reference's loop would have settled on: --coarse-freq)
    std::unique_ptr<Filter_FIR_hip>              matched_flt  (new Filter_FIR_hip(ctx, N_pl * osf));
    std::unique_ptr<Sync_timing_perfect>         sync_timing_p(stm_fast ? nullptr : new Sync_timing_perfect(N_pl * osf, osf, F));   // the default: a known phase
    std::unique_ptr<Synchronizer_timing_hip<>>   sync_timing  (stm_fast ? new Synchronizer_timing_hip<>(ctx, 0.70710678f, 5e-5f, 2.f, stm_ultra ? DVBS2HIP_STM_ULTRA : DVBS2HIP_STM_FAST, stm_hold_size) : nullptr);   // --stm-type FAST | ULTRA (Gardner)
    std::unique_ptr<Synchronizer_frame_hip<>>    sync_frame   (new Synchronizer_frame_hip<>(ctx));
    std::unique_ptr<Scrambler_PL_hip>            pl_scrambler (new Scrambler_PL_hip(ctx));
    std::unique_ptr<Synchronizer_freq_fine_hip<>> sync_fine_lr(new Synchronizer_freq_fine_hip<>(ctx, true));
    std::unique_ptr<Synchronizer_freq_fine_hip<>> sync_fine_pf(new Synchronizer_freq_fine_hip<>(ctx, false));
    std::unique_ptr<Framer_hip>                  framer       (new Framer_hip(ctx));
    std::unique_ptr<Estimator_hip>               estimator    (new Estimator_hip(ctx));
    std::unique_ptr<Modem_hip<>>                 modem        (new Modem_hip<>(ctx));
    std::unique_ptr<Interleaver_hip>             itl_rx       (new Interleaver_hip(ctx));
    std::unique_ptr<Decoder_LDPC_hip<>>          LDPC_decoder (new Decoder_LDPC_hip<>(ctx));
    std::unique_ptr<Decoder_BCH_hip<>>           BCH_decoder  (new Decoder_BCH_hip<>(ctx));
    std::unique_ptr<Scrambler_BB_hip<>>          bb_scrambler (new Scrambler_BB_hip<>(ctx));
    std::unique_ptr<Monitor_BFER_hip<>>          monitor      (new Monitor_BFER_hip<>(ctx));
    std::unique_ptr<spu::module::Source_file>    source       (new spu::module::Source_file(ctx->sz.K_bch, F, src_path, src_delay));
    spu::module::Probe_value<int32_t> prb_bfer_be(1, "BE", F);                   // main_sched.cpp:153-156
    spu::module::Probe_value<int32_t> prb_bfer_fe(1, "FE", F);
    spu::module::Probe_value<float> prb_bfer_ber(1, "BER", F);
    spu::module::Probe_value<float> prb_bfer_fer(1, "FER", F);

    (*front_agc    )[             mlt::sck::imultiply    ::X_N     ] = rx_samples;                                                                 // main_sched.cpp:197 (producer = the radio's socket)
    (*sync_coarse_f)[             sfc::sck::synchronize  ::X_N1    ] = (*front_agc    )[             mlt::sck::imultiply    ::Z_N     ];   // main_sched.cpp:198
    (*matched_flt  )[             flt::sck::filter1      ::X_N1    ] = (*sync_coarse_f)[             sfc::sck::synchronize  ::Y_N2    ];   // main_sched.cpp:199
    (*matched_flt  )[             flt::sck::filter2      ::X_N1    ] = (*sync_coarse_f)[             sfc::sck::synchronize  ::Y_N2    ];   // main_sched.cpp:200
    (*matched_flt  )[             flt::sck::filter2      ::Y_N2h   ] = (*matched_flt  )[             flt::sck::filter1      ::Y_N2    ];   // main_sched.cpp:201
    if (stm_fast) {
    (*sync_timing  )[             stm::sck::synchronize  ::X_N1    ] = (*matched_flt  )[             flt::sck::filter2      ::Y_N2    ];   // main_sched.cpp:202
    (*sync_timing  )[             stm::sck::extract      ::B_N1    ] = (*sync_timing  )[             stm::sck::synchronize  ::B_N1    ];   // main_sched.cpp:203
    (*sync_timing  )[             stm::sck::extract      ::Y_N1    ] = (*sync_timing  )[             stm::sck::synchronize  ::Y_N1    ];   // main_sched.cpp:204
    (*mult_agc     )[             mlt::sck::imultiply    ::X_N     ] = (*sync_timing  )[             stm::sck::extract      ::Y_N2    ];   // main_sched.cpp:205
    } else {
    sync_timing_p->in() = (*matched_flt)[             flt::sck::filter2      ::Y_N2    ];                                                // stand-in for :202-204 (a known phase)
    (*mult_agc     )[             mlt::sck::imultiply    ::X_N     ] = sync_timing_p->out();                                            // main_sched.cpp:205, producer = the stand-in
    }
    (*sync_frame   )[             sfm::sck::synchronize1 ::X_N1    ] = (*mult_agc     )[             mlt::sck::imultiply    ::Z_N     ];   // main_sched.cpp:206
    (*sync_frame   )[             sfm::sck::synchronize2 ::X_N1    ] = (*mult_agc     )[             mlt::sck::imultiply    ::Z_N     ];   // main_sched.cpp:207
    (*sync_frame   )[             sfm::sck::synchronize2 ::cor_SOF ] = (*sync_frame   )[             sfm::sck::synchronize1 ::cor_SOF ];   // main_sched.cpp:208
    (*sync_frame   )[             sfm::sck::synchronize2 ::cor_PLSC] = (*sync_frame   )[             sfm::sck::synchronize1 ::cor_PLSC];   // main_sched.cpp:209
    (*pl_scrambler )[             scr::sck::descramble   ::Y_N1    ] = (*sync_frame   )[             sfm::sck::synchronize2 ::Y_N2    ];   // main_sched.cpp:210
    (*sync_fine_lr )[             sff::sck::synchronize  ::X_N1    ] = (*pl_scrambler )[             scr::sck::descramble   ::Y_N2    ];   // main_sched.cpp:211
    (*sync_fine_pf )[             sff::sck::synchronize  ::X_N1    ] = (*sync_fine_lr )[             sff::sck::synchronize  ::Y_N2    ];   // main_sched.cpp:212
    (*framer       )[             frm::sck::remove_plh   ::Y_N1    ] = (*sync_fine_pf )[             sff::sck::synchronize  ::Y_N2    ];   // main_sched.cpp:213
    (*estimator    )[             est::sck::estimate     ::X_N     ] = (*framer       )[             frm::sck::remove_plh   ::Y_N2    ];   // main_sched.cpp:214
    (*modem        )[             mdm::sck::demodulate   ::CP      ] = (*estimator    )[             est::sck::estimate     ::SIG     ];   // main_sched.cpp:215
    (*modem        )[             mdm::sck::demodulate   ::Y_N1    ] = (*framer       )[             frm::sck::remove_plh   ::Y_N2    ];   // main_sched.cpp:216
    (*itl_rx       )[             itl::sck::deinterleave ::itl     ] = (*modem        )[             mdm::sck::demodulate   ::Y_N2    ];   // main_sched.cpp:217
    (*LDPC_decoder )[             dec::sck::decode_siho  ::Y_N     ] = (*itl_rx       )[             itl::sck::deinterleave ::nat     ];   // main_sched.cpp:218
    (*BCH_decoder  )[             dec::sck::decode_hiho  ::Y_N     ] = (*LDPC_decoder )[             dec::sck::decode_siho  ::V_K     ];   // main_sched.cpp:219
    (*bb_scrambler )[             scr::sck::descramble   ::Y_N1    ] = (*BCH_decoder  )[             dec::sck::decode_hiho  ::V_K     ];   // main_sched.cpp:220
    (*monitor      )[             mnt::sck::check_errors2::U       ] = (*source       )[spu::module::src::sck::generate     ::out_data];   // main_sched.cpp:221
    (*monitor      )[             mnt::sck::check_errors2::V       ] = (*bb_scrambler )[             scr::sck::descramble   ::Y_N2    ];   // main_sched.cpp:222
    prb_bfer_be     [spu::module::prb::sck::probe        ::in      ] = (*monitor      )[             mnt::sck::check_errors2::BE      ];   // main_sched.cpp:244
    prb_bfer_fe     [spu::module::prb::sck::probe        ::in      ] = (*monitor      )[             mnt::sck::check_errors2::FE      ];   // main_sched.cpp:245
    prb_bfer_ber    [spu::module::prb::sck::probe        ::in      ] = (*monitor      )[             mnt::sck::check_errors2::BER     ];   // main_sched.cpp:246
    prb_bfer_fer    [spu::module::prb::sck::probe        ::in      ] = (*monitor      )[             mnt::sck::check_errors2::FER     ];   // main_sched.cpp:247

    std::vector<spu::runtime::Task *> timing_tasks;
    if (stm_fast) timing_tasks = {&(*sync_timing)[stm::tsk::synchronize], &(*sync_timing)[stm::tsk::extract]};
    else timing_tasks = {&(*sync_timing_p)()};
    std::vector<spu::runtime::Task *> order = {&(*front_agc)(), &(*sync_coarse_f)(), &(*matched_flt)[flt::tsk::filter1],
                                               &(*matched_flt)[flt::tsk::filter2]};
    order.insert(order.end(), timing_tasks.begin(), timing_tasks.end());
    spu::runtime::Sequence seq(order);
    // the tasks behind the timing synchronizer: a batch whose extract underflows ends there (the reference's sequence stops at a processing_aborted task)
    spu::runtime::Sequence seq2({&(*source)[spu::module::src::tsk::generate], &(*mult_agc)(), &(*sync_frame)[sfm::tsk::synchronize1], &(*sync_frame)[sfm::tsk::synchronize2], &(*pl_scrambler)(),
                                &(*sync_fine_lr)(), &(*sync_fine_pf)(), &(*framer)(), &(*estimator)(), &(*modem)(), &(*itl_rx)(), &(*LDPC_decoder)(),
                                &(*BCH_decoder)(), &(*bb_scrambler)(), &(*monitor)[mnt::tsk::check_errors2], &prb_bfer_be[spu::module::prb::tsk::probe],
                                &prb_bfer_fe[spu::module::prb::tsk::probe], &prb_bfer_ber[spu::module::prb::tsk::probe], &prb_bfer_fer[spu::module::prb::tsk::probe]});

    std::ifstream in(in_path, std::ios::binary);
    if (!in) throw spu::tools::runtime_error(__FILE__, __LINE__, __func__, "cannot open " + in_path);
    std::ofstream out;
    if (!out_path.empty()) out.open(out_path, std::ios::binary);
    size_t batches = 0;
    size_t aborted = 0;
    if (wl_phases) {
        // the waiting and learning phases of RX/main_sched.cpp:407-635 on the head of the file
        namespace fbr = spu::module::fbr;
        std::unique_ptr<Synchronizer_step_mf_hip<>> sync_step_mf(new Synchronizer_step_mf_hip<>(sync_coarse_f.get(), matched_flt.get(), sync_timing.get(), ctx));
        if (smf_kernel >= 0) sync_step_mf->set_kernel(smf_kernel);                                                   // --smf-kernel
        std::unique_ptr<spu::module::Feedbacker<int>> feedbr(new spu::module::Feedbacker<int>(1, 0, F));
        // partial binding
        (*sync_step_mf)[             smf::sck::synchronize::X_N1] = (*front_agc   )[mlt::sck::imultiply   ::Z_N ];   // main_sched.cpp:428
        (*sync_step_mf)[             smf::sck::synchronize::DEL ] = (*feedbr      )[fbr::sck::produce     ::Y_N ];   // main_sched.cpp:429
        (*feedbr      )[             fbr::sck::memorize   ::X_N ] = (*sync_frame  )[sfm::sck::synchronize2::DEL ];   // main_sched.cpp:430
        (*sync_timing )[             stm::sck::extract    ::B_N1] = (*sync_step_mf)[smf::sck::synchronize ::B_N1];   // main_sched.cpp:431
        (*sync_timing )[             stm::sck::extract    ::Y_N1] = (*sync_step_mf)[smf::sck::synchronize ::Y_N1];   // main_sched.cpp:432
        // the sequence from the radio to the Feedbacker's memorize (firsts / lasts of main_sched.cpp:438-454); an underflowing extract cuts an iteration short
        spu::runtime::Sequence wl12a({&(*feedbr)[fbr::tsk::produce], &(*front_agc)(), &(*sync_step_mf)[smf::tsk::synchronize], &(*sync_timing)[stm::tsk::extract]});
        spu::runtime::Sequence wl12b({&(*mult_agc)(), &(*sync_frame)[sfm::tsk::synchronize1], &(*sync_frame)[sfm::tsk::synchronize2], &(*feedbr)[fbr::tsk::memorize]});
        auto wl12_step = [&]() -> bool {
            if (!in.read(reinterpret_cast<char *>(rx_samples.data()), rx_samples.size() * sizeof(float))) return false;
            try { wl12a.exec_step(); } catch (const spu::tools::processing_aborted &) { return true; }
            wl12b.exec_step();
            return true;
        };
        int waited = 0;
        bool more = true, flag = false;
        sync_coarse_f->set_PLL_coeffs(1, 1 / std::sqrt(2.0), 1e-4);                                                   // main_sched.cpp:472
        while (!flag && waited < wl_wait_max && (more = wl12_step())) { waited += F; flag = sync_frame->get_packet_flag(); }      // :478-494
        if (!flag) { std::printf("# waiting phase gave up after %d frames\n", waited); return 4; }
        sync_step_mf->reset();                                                                                       // main_sched.cpp:500
        sync_frame  ->reset();                                                                                       // main_sched.cpp:501
        sync_timing ->reset();                                                                                       // main_sched.cpp:502
        int m = 0, limit = wl1;
        bool second = false;
        sync_coarse_f->set_PLL_coeffs(1, 1 / std::sqrt(2.0), 1e-4);                                                   // main_sched.cpp:529
        while (m < limit && (more = wl12_step())) {                                                                  // :535-560
            m += F;
            if (!second && m >= wl1) { second = true; limit = m + wl2; sync_coarse_f->set_PLL_coeffs(1, 1 / std::sqrt(2.0), 5e-5); }      // :548-558
        }
        const int learned12 = m;
        // learning phase 3: partial binding back to the steady-state graph
        (*sync_coarse_f)[             sfc::sck::synchronize::X_N1] = (*front_agc    )[mlt::sck::imultiply  ::Z_N ];   // main_sched.cpp:576
        (*sync_timing  )[             stm::sck::extract    ::B_N1] = (*sync_timing  )[stm::sck::synchronize::B_N1];   // main_sched.cpp:577
        (*sync_timing  )[             stm::sck::extract    ::Y_N1] = (*sync_timing  )[stm::sck::synchronize::Y_N1];   // main_sched.cpp:578
        spu::runtime::Sequence l3({&(*mult_agc)(), &(*sync_frame)[sfm::tsk::synchronize1], &(*sync_frame)[sfm::tsk::synchronize2], &(*pl_scrambler)(), &(*sync_fine_lr)(),
                                   &(*sync_fine_pf)()});                                                            // up to lasts_l3, main_sched.cpp:595
        m = 0;
        while (more && m < wl3 && in.read(reinterpret_cast<char *>(rx_samples.data()), rx_samples.size() * sizeof(float))) {      // :613-630
            m += F;
            try { seq.exec_step(); } catch (const spu::tools::processing_aborted &) { continue; }
            l3.exec_step();
        }
        std::printf("# wl phases | waiting %d | learning %d + %d frames | coarse frequency %.6f\n", waited, learned12, m, (double)sync_coarse_f->get_estimated_freq());
    }
    size_t fed = 0;                                                       // frames the timing synchronizer has taken
    while (in.read(reinterpret_cast<char *>(rx_samples.data()), rx_samples.size() * sizeof(float))) {
        if (stm_ultra && fed >= (size_t)stm_learn_frames) sync_timing->set_act(true);      // the learning frames are over: the loop holds (main_sched.cpp:655)
        fed += (size_t)F;
        try {
            seq.exec_step();
        } catch (const spu::tools::processing_aborted &) {
            aborted++;                  // too few symbols for F frames: they wait in the synchronizer for the next batch
            continue;
        }
        seq2.exec_step();
        if ((int)batches < mon_skip) monitor->reset();       // the synchronizers are still locking: keep these batches out of the statistics (the reference's waiting and learning phases)
        // The fine frequency estimate of ONE frame is noisy (sigma ~2.5e-4 cycles per symbol at 16 dB against the +-3.4e-4 the pilot-aided stage can take back): it lives on its memory of
        // alpha = 0.999.  In the reference the fine synchronizers do not run before the frame synchronizer has locked -- its learning phases 1 and 2 end at sync_frame
        // (main_sched.cpp:454,535) -- and then settle for a learning phase 3 (:597-630) before anything is counted.  Here: the first half of --mon-skip is phases 1 and 2 (what the
        // estimate saw of the unaligned frames is dropped), the second half is phase 3.
        if (!wl_phases && (int)batches < (mon_skip + 1) / 2) sync_fine_lr->reset();
        if (out.is_open())
            out.write(reinterpret_cast<const char *>((*bb_scrambler)[scr::sck::descramble::Y_N2].get_dataptr<int>()), (size_t)F * ctx->sz.K_bch * sizeof(int));
        batches++;
    }
    uint64_t fra = 0, be = 0, fe = 0;
    monitor->get(fra, be, fe);
    std::printf("# %s F=%d %s ite=%d matched-filter graph | batches %zu | FRA %llu BE %llu FE %llu\n", modcod.c_str(), F, implem.c_str(), n_ite, batches,
                (unsigned long long)fra, (unsigned long long)be, (unsigned long long)fe);
    if (stm_ultra) std::printf("# timing ULTRA hold size %d, holding after %d frames | batches aborted by an underflow %zu\n", stm_hold_size, stm_learn_frames, aborted);
    else if (stm_fast) std::printf("# timing FAST | batches aborted by an underflow %zu\n", aborted);
    std::printf("# probes | BE %d FE %d BER %.3e FER %.3e | DEL %d FLG %d\n", prb_bfer_be.last, prb_bfer_fe.last, (double)prb_bfer_ber.last, (double)prb_bfer_fer.last,
                (*sync_frame)[sfm::sck::synchronize2::DEL].get_dataptr<int>()[F - 1], (*sync_frame)[sfm::sck::synchronize2::FLG].get_dataptr<int>()[F - 1]);
    return 0;
}

int main(int argc, char **argv)
{
    std::string modcod = "QPSK-S_8/9", in_path, out_path, src_path, implem = "SPA";     // DVBS2.cpp:135-138: SPA, 50 iterations
    int F = 1, n_ite = 50, src_delay = 0, mon_skip = 0;
    float coarse_freq = 0.f;
    float alpha = 1.0f;
    bool frame_sync = false, matched = false, stm_fast = false, stm_ultra = false, wl_phases = false;
    int wl[3] = {150, 150, 200}, wl_wait_max = 2000, stm_hold_size = 101, stm_learn_frames = -1, smf_kernel = -1;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) { std::cerr << "missing value for " << a << "\n"; exit(2); } return argv[++i]; };
        if (a == "--mod-cod") modcod = next();
        else if (a == "-F" || a == "--sim-inter-fra") F = std::stoi(next());
        else if (a == "--dec-ite") n_ite = std::stoi(next());
        else if (a == "--dec-implem") implem = next();
        else if (a == "--dec-alpha") alpha = std::stof(next());
        else if (a == "--in") in_path = next();
        else if (a == "--out") out_path = next();
        else if (a == "--src") src_path = next();
        else if (a == "--src-delay") src_delay = std::stoi(next());
        else if (a == "--mon-skip") mon_skip = std::stoi(next());
        else if (a == "--coarse-freq") coarse_freq = std::stof(next());      // normalized frequency offset of the received samples (cycles per sample): the coarse synchronizer's frozen estimate
        else if (a == "--wl-phases") wl_phases = true;                         // the waiting and learning phases on the head of the file (main_sched.cpp:407-635)
        else if (a == "--wl-frames") { for (int &w : wl) w = std::stoi(next()); }
        else if (a == "--wl-wait-max") wl_wait_max = std::stoi(next());
        else if (a == "--smf-kernel") {
            const std::string t = next();
            if (t != "LANE" && t != "WAVE") { std::cerr << "--smf-kernel: LANE or WAVE\n"; return 2; }
            smf_kernel = t == "WAVE" ? DVBS2HIP_SMF_WAVE : DVBS2HIP_SMF_LANE;
        }
        else if (a == "--frame-sync") frame_sync = true;
        else if (a == "--matched-filter") matched = true;
        else if (a == "--stm-type") {
            const std::string t = next();
            if (t != "PERFECT" && t != "FAST" && t != "ULTRA") { std::cerr << "--stm-type: PERFECT, FAST or ULTRA\n"; return 2; }
            stm_ultra = t == "ULTRA"; stm_fast = t != "PERFECT";        // stm_fast: the timing module is bound; stm_ultra: as Synchronizer_Gardner_ultra_osf2
        }
        else if (a == "--stm-hold-size") stm_hold_size = std::stoi(next());
        else if (a == "--stm-learn-frames") stm_learn_frames = std::stoi(next());      // ULTRA: frames before set_act(true); default: the sum of --wl-frames
        else { std::cerr << "unknown argument " << a << "\n"; return 2; }
    }
    try {
        if (stm_fast && !matched) { std::cerr << "--stm-type FAST | ULTRA needs --matched-filter (the timing synchronizer runs on the samples)\n"; return 2; }
        if (stm_ultra && stm_hold_size <= 4) { std::cerr << "--stm-hold-size has to be greater than 4\n"; return 2; }
        if (stm_ultra && wl_phases) { std::cerr << "--wl-phases steps FAST's detector inside the coarse-frequency loop: with --stm-type ULTRA it is not provided (use --stm-learn-frames)\n"; return 2; }
        if (smf_kernel >= 0 && !wl_phases) { std::cerr << "--smf-kernel chooses the kernel of the coarse-frequency loop, which only --wl-phases runs: give both or neither\n"; return 2; }
        if (stm_learn_frames < 0) stm_learn_frames = wl[0] + wl[1] + wl[2];
        if (wl_phases && (!stm_fast || coarse_freq != 0.f)) { std::cerr << "--wl-phases needs --matched-filter --stm-type FAST and excludes --coarse-freq\n"; return 2; }
        if (matched) return run_matched_filter_graph(modcod, F, n_ite, alpha, implem, in_path, out_path, src_path, src_delay, mon_skip, coarse_freq, stm_fast, wl_phases,
                                                     wl[0], wl[1], wl[2], wl_wait_max, stm_ultra, stm_hold_size, stm_learn_frames, smf_kernel);
        auto ctx = std::make_shared<module::Context>(modcod, F, n_ite, alpha, true, 0, implem);
        ctx->pin_sockets = true;            // the sockets below live until the modules go: pin them for overlapped PCIe copies
        module::Scrambler_PL_hip pl_scrambler(ctx);
        module::Framer_hip framer(ctx);
        module::Estimator_hip estimator(ctx);
        module::Modem_hip<> modem(ctx);
        module::Interleaver_hip itl_rx(ctx);
        module::Decoder_LDPC_hip<> LDPC_decoder(ctx);
        module::Decoder_BCH_hip<> BCH_decoder(ctx);
        module::Scrambler_BB_hip<> bb_scrambler(ctx);
        module::Monitor_BFER_hip<> monitor(ctx);
        module::Receiver_BB_hip<> receiver(ctx);

        std::vector<float> pl_frames((size_t)F * 2 * ctx->sz.pl_frame_sym);
        std::vector<int> sent((size_t)F * ctx->sz.K_bch, 0);

        // socket binding, as TX_RX_BB/main.cpp:83-94 (RX side)
        using namespace module;
        pl_scrambler[scr::sck::descramble::Y_N1] = pl_frames;
        framer      [frm::sck::remove_plh::Y_N1] = pl_scrambler[scr::sck::descramble::Y_N2];
        estimator   [est::sck::estimate::X_N   ] = framer      [frm::sck::remove_plh::Y_N2];
        modem       [mdm::sck::demodulate::CP  ] = estimator   [est::sck::estimate::SIG   ];
        modem       [mdm::sck::demodulate::Y_N1] = framer      [frm::sck::remove_plh::Y_N2];
        itl_rx      [itl::sck::deinterleave::itl] = modem      [mdm::sck::demodulate::Y_N2];
        LDPC_decoder[dec::sck::decode_siho::Y_N] = itl_rx      [itl::sck::deinterleave::nat];
        BCH_decoder [dec::sck::decode_hiho::Y_N] = LDPC_decoder[dec::sck::decode_siho::V_K];
        bb_scrambler[scr::sck::descramble::Y_N1] = BCH_decoder [dec::sck::decode_hiho::V_K];
        monitor     [mnt::sck::check_errors::U ] = sent;
        monitor     [mnt::sck::check_errors::V ] = bb_scrambler[scr::sck::descramble::Y_N2];
        receiver    [rcv::sck::receive::Y_N1   ] = pl_frames;

        std::vector<spu::runtime::Task *> order = {&pl_scrambler(), &framer(), &estimator(), &modem(), &itl_rx(),
                                                   &LDPC_decoder(), &BCH_decoder(), &bb_scrambler()};
        std::unique_ptr<module::Synchronizer_frame_hip<>> sync_frame;
        if (frame_sync) {
            sync_frame.reset(new module::Synchronizer_frame_hip<>(ctx));
            (*sync_frame)[sfm::sck::synchronize::X_N1] = pl_frames;
            pl_scrambler[scr::sck::descramble::Y_N1] = (*sync_frame)[sfm::sck::synchronize::Y_N2];
            receiver    [rcv::sck::receive::Y_N1   ] = (*sync_frame)[sfm::sck::synchronize::Y_N2];
            order.insert(order.begin(), &(*sync_frame)[sfm::tsk::synchronize]);
        }
        if (!src_path.empty()) order.push_back(&monitor[mnt::tsk::check_errors]);
        spu::runtime::Sequence seq(order);

        std::ifstream in(in_path, std::ios::binary);
        if (!in) throw spu::tools::runtime_error(__FILE__, __LINE__, __func__, "cannot open " + in_path);
        std::ifstream src;
        if (!src_path.empty()) { src.open(src_path, std::ios::binary); if (!src) throw spu::tools::runtime_error(__FILE__, __LINE__, __func__, "cannot open " + src_path); }
        std::ofstream out;
        if (!out_path.empty()) out.open(out_path, std::ios::binary);

        size_t batches = 0, mismatch = 0;
        while (in.read(reinterpret_cast<char *>(pl_frames.data()), pl_frames.size() * sizeof(float))) {
            if (src.is_open()) src.read(reinterpret_cast<char *>(sent.data()), sent.size() * sizeof(int));
            seq.exec_step();            // the reference's graph, one task per codelet
            receiver().exec();          // the fused device-resident chain
            const int *a = bb_scrambler[scr::sck::descramble::Y_N2].get_dataptr<int>();
            const int *b = receiver[rcv::sck::receive::V_K].get_dataptr<int>();
            for (size_t i = 0; i < sent.size(); i++) mismatch += a[i] != b[i];
            if (out.is_open()) out.write(reinterpret_cast<const char *>(b), sent.size() * sizeof(int));
            batches++;
        }
        uint64_t fra = 0, be = 0, fe = 0;
        monitor.get(fra, be, fe);
        std::printf("# %s F=%d %s ite=%d | batches %zu | task-graph vs fused mismatches %zu | FRA %llu BE %llu FE %llu\n", modcod.c_str(), F, implem.c_str(),
                    n_ite, batches, mismatch, (unsigned long long)fra, (unsigned long long)be, (unsigned long long)fe);
        if (sync_frame)
            std::printf("# frame-sync | DEL %d FLG %d TRI %.3f\n", (*sync_frame)[sfm::sck::synchronize::DEL].get_dataptr<int>()[F - 1],
                        (*sync_frame)[sfm::sck::synchronize::FLG].get_dataptr<int>()[F - 1], (double)(*sync_frame)[sfm::sck::synchronize::TRI].get_dataptr<float>()[F - 1]);
        return mismatch ? 1 : 0;
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return 3;
    }
}
