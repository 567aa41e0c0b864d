// Every run-time switch the library reads from the environment, in one place. Each accessor reads
// its variable once per process, on first use, and keeps the answer; INTEGRATION.md ("Run-time
// switches") carries the same list as a table, and tests/test_host.py holds the two together.
#pragma once
#include <cstdlib>
#include <string>

namespace sw {

// ---- the three on / off rules in use, and the two value forms
// unset: `dflt`; set: on unless it parses to 0 (std::atoi, so "" and text count as 0)
inline bool on_unless_zero(const char* name, bool dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) != 0 : dflt;
}
// on unless the value parses to exactly 1 (unset included)
inline bool on_unless_one(const char* name) {
  const char* e = std::getenv(name);
  return !e || std::atoi(e) != 1;
}
// on when the variable exists at all, whatever it holds: NAME=0 and NAME= are both "on"
inline bool present(const char* name) { return std::getenv(name) != nullptr; }
// integer value (std::atoi), `dflt` when unset
inline int number(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}
// the text itself, "" when unset
inline std::string text(const char* name) {
  const char* e = std::getenv(name);
  return e ? e : "";
}

// ---- context
// TTS_GEMM=f32 starts every context on the fp32 GEMM kernels (default: split-f16)
inline bool gemm_f32() { static const bool v = text("TTS_GEMM") == "f32"; return v; }
// TTS_VOC_STREAM=0 runs the vocoder on the library stream instead of a second one
inline bool voc_stream() { static const bool v = on_unless_zero("TTS_VOC_STREAM", true); return v; }

// ---- grid barriers
// TTS_BARRIER_TIMEOUT_MS: wait limit of a grid barrier, clamped to [1, 40000] ms (default 2000)
inline double barrier_timeout_ms() {
  static const double v = [] {
    const char* e = std::getenv("TTS_BARRIER_TIMEOUT_MS");
    const double ms = e ? std::atof(e) : 2000.0;
    return ms < 1.0 ? 1.0 : (ms > 40000.0 ? 40000.0 : ms);
  }();
  return v;
}
// TTS_COOP_LAUNCH=1 launches the grid-barrier kernels with hipLaunchCooperativeKernel
inline bool coop_launch() { static const bool v = on_unless_zero("TTS_COOP_LAUNCH", false); return v; }
// TTS_BAR_CALIBRATE=0 takes the first barrier blocks of the pool instead of timing the candidates
inline bool bar_calibrate() { static const bool v = on_unless_zero("TTS_BAR_CALIBRATE", true); return v; }
// TTS_DIAG_XCC: print the calibration's per-block times and each launch's workgroup -> XCD map
inline bool diag_xcc() { static const bool v = present("TTS_DIAG_XCC"); return v; }

// ---- Tacotron2
// TTS_ENCODER=steps: per-step BiLSTM launches instead of the one persistent launch
inline bool encoder_steps() { static const bool v = text("TTS_ENCODER") == "steps"; return v; }
// TTS_LSTM_RG=1 turns the BiLSTM's row groups off
inline bool lstm_row_groups() { static const bool v = on_unless_one("TTS_LSTM_RG"); return v; }
// TTS_DECODER=graph: the captured-graph decoder instead of the persistent kernel
inline bool decoder_graph() { static const bool v = text("TTS_DECODER") == "graph"; return v; }
// TTS_DECODER_F32 (present at all): the persistent decoder's GEMM parts on the fp32 MFMA
inline bool decoder_f32() { static const bool v = present("TTS_DECODER_F32"); return v; }
// TTS_ALIGN_IN_P4 (present at all): the old alignment pass in phase 4 instead of the deferred one,
// in which each item workgroup writes its own positions in phase 6
inline bool align_in_p4() { static const bool v = present("TTS_ALIGN_IN_P4"); return v; }
// TTS_PTRACE=<file>: phase timestamps of 8 decoder steps, written to <file> (a library built with
// -DTTS_PHASE_TRACE); nullptr when unset
inline const char* ptrace_file() {
  static const bool set = present("TTS_PTRACE");
  static const std::string v = text("TTS_PTRACE");
  return set ? v.c_str() : nullptr;
}
// TTS_PTRACE_T0: first traced step (default 100)
inline int ptrace_t0() { static const int v = number("TTS_PTRACE_T0", 100); return v; }
// TTS_PTRACE_LAUNCH: which launch of the MT cascade is traced (default 0, the first)
inline int ptrace_launch() { static const int v = number("TTS_PTRACE_LAUNCH", 0); return v; }

// ---- MB-MelGAN
// TTS_STACK_FUSE=0: a C = 48 ResidualStack block by block instead of blocks 0-2 as one kernel
inline bool stack_fuse() { static const bool v = on_unless_zero("TTS_STACK_FUSE", true); return v; }
// TTS_STACK_FUSE96=1: the C = 96 stack in one launch too; off by default since round 5.
// Same-box A/B over 4 bench runs each (profiles/r05/v17_stack96_ab.txt): vocoder 2.958 ms fused
// against 2.922 ms with blocks 0-2 as three resblock_x3 launches; the stack kernel's halo
// recompute (up to 24 extra rows per 96-position tile) now costs more than the two HBM round trips
// of x it saves at this width, while at C = 48 (with the fused ConvTranspose) fusing still wins
inline bool stack_fuse96() { static const bool v = on_unless_zero("TTS_STACK_FUSE96", false); return v; }
// TTS_CT_FUSE=0 keeps the last upsample's ConvTranspose as a separate conv_x3 launch instead of
// running it inside the C = 48 stack kernel (resstack_x3.hip CTU = 2)
inline bool ct_fuse() { static const bool v = on_unless_zero("TTS_CT_FUSE", true); return v; }
// TTS_CX_NI128 = 3 / 4 forces conv_x3's 128-row tile to 48 / 64 columns (0: chosen per call)
inline int cx_ni128() { static const int v = number("TTS_CX_NI128", 0); return v; }

// ---- GE2E
// TTS_GE2E_PIPE=0 (exactly "0") keeps one launch per layer instead of the persistent pipeline
inline bool ge2e_pipe() { static const bool v = text("TTS_GE2E_PIPE") != "0"; return v; }

// ---- ParallelWaveGAN
// TTS_PWGAN_STAGING=regs / ring4: the fp32 residual-block kernel with register staging / a 4-deep
// LDS-DMA ring instead of the 3-deep ring. Returns 0 = regs, 1 = the default ring, 2 = ring4
inline int pwgan_staging() {
  static const int v = [] {
    const std::string e = text("TTS_PWGAN_STAGING");
    return e == "regs" ? 0 : e == "ring4" ? 2 : 1;
  }();
  return v;
}
// TTS_PWGAN_TILE=1 / 2: the split-f16 residual block as the per-tile kernel / the 4-wave persistent
// kernel instead of the 8-wave persistent one
inline int pwgan_tile() { static const int v = number("TTS_PWGAN_TILE", 0); return v; }

}  // namespace sw
