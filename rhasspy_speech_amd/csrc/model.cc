#include "model.h"
#include "call_plan.h"
#include "nnet3_setup.h"
#include "env.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <fstream>
#include <limits>
#include <set>
#include <sstream>

namespace rs {

// =============================================================================== options

static bool ParseBool(const std::string &v, const std::string &key) {
  if (v == "true" || v == "t" || v == "1" || v == "True" || v == "T" || v.empty()) return true;
  if (v == "false" || v == "f" || v == "0" || v == "False" || v == "F") return false;
  Fail("Invalid boolean value for --" + key + ": " + v);
}

int MfccOptions::PaddedWindowSize() const {
  int w = WindowSize();
  if (!round_pow2) return w;
  int p = 1;
  while (p < w) p <<= 1;
  return p;
}

void ReadMfccOptions(const std::string &conf_path, MfccOptions *o) {
  for (auto &kv : ReadConfigFile(conf_path)) {
    const std::string &k = kv.first, &v = kv.second;
    if (k == "sample-frequency") o->samp_freq = std::stof(v);
    else if (k == "frame-length") o->frame_length_ms = std::stof(v);
    else if (k == "frame-shift") o->frame_shift_ms = std::stof(v);
    else if (k == "preemphasis-coefficient") o->preemph = std::stof(v);
    else if (k == "remove-dc-offset") o->remove_dc = ParseBool(v, k);
    else if (k == "dither") o->dither = std::stof(v);
    else if (k == "window-type") o->window_type = v;
    else if (k == "blackman-coeff") o->blackman_coeff = std::stof(v);
    else if (k == "round-to-power-of-two") o->round_pow2 = ParseBool(v, k);
    else if (k == "snip-edges") o->snip_edges = ParseBool(v, k);
    else if (k == "allow-downsample") o->allow_downsample = ParseBool(v, k);
    else if (k == "allow-upsample") o->allow_upsample = ParseBool(v, k);
    else if (k == "max-feature-vectors" || k == "debug-mel") {}
    else if (k == "num-mel-bins") o->num_bins = std::stoi(v);
    else if (k == "low-freq") o->low_freq = std::stof(v);
    else if (k == "high-freq") o->high_freq = std::stof(v);
    else if (k == "vtln-low") o->vtln_low = std::stof(v);
    else if (k == "vtln-high") o->vtln_high = std::stof(v);
    else if (k == "num-ceps") o->num_ceps = std::stoi(v);
    else if (k == "use-energy") o->use_energy = ParseBool(v, k);
    else if (k == "energy-floor") o->energy_floor = std::stof(v);
    else if (k == "raw-energy") o->raw_energy = ParseBool(v, k);
    else if (k == "cepstral-lifter") o->cepstral_lifter = std::stof(v);
    else if (k == "htk-compat") o->htk_compat = ParseBool(v, k);
    else Fail("Invalid option --" + k + "=" + v + " in config file " + conf_path);
  }
}

int NumFrames(long num_samples, const MfccOptions &o) {
  return FramesOf(num_samples, o.WindowSize(), o.WindowShift());
}

// mel-computations.h:81-87
static inline float MelScale(float freq) { return 1127.0f * logf(1.0f + freq / 700.0f); }

// The window and the mel filters: what both feature types share (`what`: the type's name in the messages)
static void BuildFrameAndMelTables(const MfccOptions &o, const std::string &what, MfccTables *t) {
  t->opts = o;
  if (!o.snip_edges) Fail(what + ": --snip-edges=false is not supported by the HIP feature kernel");
  t->win = o.WindowSize();
  t->shift = o.WindowShift();
  t->padded = o.PaddedWindowSize();
  if (t->padded != 256 && t->padded != 512 && t->padded != 1024 && t->padded != 2048)
    Fail(what + ": padded window size " + std::to_string(t->padded) + " unsupported by the HIP FFT (need 256, 512, 1024 or 2048)");
  t->nbins = o.num_bins;
  // window (feature-window.cc:113-125): computed in double, stored as float
  t->window.resize(t->win);
  double a = 2.0 * M_PI / (t->win - 1);
  for (int i = 0; i < t->win; i++) {
    double x = (double)i, w;
    if (o.window_type == "hanning") w = 0.5 - 0.5 * cos(a * x);
    else if (o.window_type == "sine") w = sin(0.5 * a * x);
    else if (o.window_type == "hamming") w = 0.54 - 0.46 * cos(a * x);
    else if (o.window_type == "povey") w = pow(0.5 - 0.5 * cos(a * x), 0.85);
    else if (o.window_type == "rectangular") w = 1.0;
    else if (o.window_type == "blackman") w = o.blackman_coeff - 0.5 * cos(a * x) + (0.5 - o.blackman_coeff) * cos(2 * a * x);
    else Fail("Invalid window type " + o.window_type);
    t->window[i] = (float)w;
  }
  // mel banks (mel-computations.cc:33-142), float arithmetic as in the reference
  float sample_freq = o.samp_freq;
  int num_fft_bins = t->padded / 2;
  float nyquist = 0.5f * sample_freq;
  float low_freq = o.low_freq, high_freq = o.high_freq > 0.0f ? o.high_freq : nyquist + o.high_freq;
  if (low_freq < 0.0f || low_freq >= nyquist || high_freq <= 0.0f || high_freq > nyquist || high_freq <= low_freq)
    Fail("Bad values in options: low-freq " + std::to_string(low_freq) + " and high-freq " + std::to_string(high_freq));
  float fft_bin_width = sample_freq / t->padded;
  float mel_low = MelScale(low_freq), mel_high = MelScale(high_freq);
  float mel_delta = (mel_high - mel_low) / (o.num_bins + 1);
  t->mel_offset.assign(o.num_bins, 0);
  t->mel_len.assign(o.num_bins, 0);
  t->mel_start.assign(o.num_bins, 0);
  t->mel_weights.clear();
  for (int bin = 0; bin < o.num_bins; bin++) {
    float left = mel_low + bin * mel_delta, center = mel_low + (bin + 1) * mel_delta, right = mel_low + (bin + 2) * mel_delta;
    std::vector<float> this_bin(num_fft_bins, 0.0f);
    int first = -1, last = -1;
    for (int i = 0; i < num_fft_bins; i++) {
      float freq = fft_bin_width * i;
      float mel = MelScale(freq);
      if (mel > left && mel < right) {
        float w;
        if (mel <= center) w = (mel - left) / (center - left);
        else w = (right - mel) / (right - center);
        this_bin[i] = w;
        if (first == -1) first = i;
        last = i;
      }
    }
    if (first == -1) Fail("You may have set --num-mel-bins too large.");
    t->mel_offset[bin] = first;
    t->mel_len[bin] = last + 1 - first;
    t->mel_start[bin] = (int)t->mel_weights.size();
    t->mel_weights.insert(t->mel_weights.end(), this_bin.begin() + first, this_bin.begin() + last + 1);
  }
  t->log_energy_floor = o.energy_floor > 0.0f ? logf(o.energy_floor) : -std::numeric_limits<float>::infinity();
}

void BuildMfccTables(const MfccOptions &o, MfccTables *t) {
  if (o.htk_compat) Fail("mfcc: --htk-compat=true is not supported by the HIP feature kernel");
  if (o.num_ceps > o.num_bins) Fail("num-ceps cannot be larger than num-mel-bins.");
  if (o.num_bins > 64 || o.num_ceps > 64) Fail("mfcc: more than 64 mel bins / cepstra are not supported by the HIP kernel");
  BuildFrameAndMelTables(o, "mfcc", t);
  t->nceps = o.num_ceps;
  // DCT (matrix-functions.cc:592-608): rows k of an N x N type-II DCT, first num_ceps rows kept
  int N = o.num_bins;
  t->dct.assign((size_t)o.num_ceps * N, 0.0f);
  {
    double normalizer = std::sqrt(1.0 / (double)N);
    for (int j = 0; j < N; j++) t->dct[j] = (float)normalizer;
    normalizer = std::sqrt(2.0 / (double)N);
    for (int k = 1; k < o.num_ceps; k++)
      for (int n = 0; n < N; n++) t->dct[(size_t)k * N + n] = (float)(normalizer * cos((double)M_PI / N * (n + 0.5) * k));
  }
  t->lifter.assign(o.num_ceps, 1.0f);
  if (o.cepstral_lifter != 0.0f)
    for (int i = 0; i < o.num_ceps; i++)
      t->lifter[i] = (float)(1.0 + 0.5 * o.cepstral_lifter * sin(M_PI * i / o.cepstral_lifter));
}

// feature-fbank.h:62-80 on top of the frame and mel options (feature-window.h:77-113, mel-computations.h:60-75).  The warping
// factor is always 1, so --vtln-low / --vtln-high at their defaults change nothing; other values, and --debug-mel, are refused.
void ReadFbankOptions(const std::string &conf_path, FbankOptions *o) {
  for (auto &kv : ReadConfigFile(conf_path)) {
    const std::string &k = kv.first, &v = kv.second;
    if (k == "sample-frequency") o->samp_freq = std::stof(v);
    else if (k == "frame-length") o->frame_length_ms = std::stof(v);
    else if (k == "frame-shift") o->frame_shift_ms = std::stof(v);
    else if (k == "preemphasis-coefficient") o->preemph = std::stof(v);
    else if (k == "remove-dc-offset") o->remove_dc = ParseBool(v, k);
    else if (k == "dither") o->dither = std::stof(v);
    else if (k == "window-type") o->window_type = v;
    else if (k == "blackman-coeff") o->blackman_coeff = std::stof(v);
    else if (k == "round-to-power-of-two") o->round_pow2 = ParseBool(v, k);
    else if (k == "snip-edges") o->snip_edges = ParseBool(v, k);
    else if (k == "allow-downsample") o->allow_downsample = ParseBool(v, k);
    else if (k == "allow-upsample") o->allow_upsample = ParseBool(v, k);
    else if (k == "max-feature-vectors") {}
    else if (k == "num-mel-bins") o->num_bins = std::stoi(v);
    else if (k == "low-freq") o->low_freq = std::stof(v);
    else if (k == "high-freq") o->high_freq = std::stof(v);
    else if (k == "vtln-low" || k == "vtln-high") {
      const float def = k == "vtln-low" ? o->vtln_low : o->vtln_high;
      if (std::stof(v) != def) Fail("fbank: --" + k + "=" + v + " is not supported by the HIP feature kernel (no VTLN warping)");
    }
    else if (k == "debug-mel") { if (ParseBool(v, k)) Fail("fbank: --debug-mel=true is not supported by the HIP feature kernel"); }
    else if (k == "use-energy") o->use_energy = ParseBool(v, k);
    else if (k == "energy-floor") o->energy_floor = std::stof(v);
    else if (k == "raw-energy") o->raw_energy = ParseBool(v, k);
    else if (k == "htk-compat") o->htk_compat = ParseBool(v, k);
    else if (k == "use-log-fbank") o->use_log_fbank = ParseBool(v, k);
    else if (k == "use-power") o->use_power = ParseBool(v, k);
    else Fail("Invalid option --" + k + "=" + v + " in config file " + conf_path);
  }
}

void BuildFbankTables(const FbankOptions &o, MfccTables *t) {
  if (o.num_bins < 3) Fail("Must have at least 3 mel bins");      // mel-computations.cc:39-40
  BuildFrameAndMelTables(o, "fbank", t);      // (too many bins for the FFT's resolution fail here, in the reference's words)
  if (o.Dim() > 128)
    Fail("fbank: " + std::to_string(o.Dim()) + " feature columns (--num-mel-bins=" + std::to_string(o.num_bins) +
         (o.use_energy ? " and the energy" : "") + ") are more than the 128 the HIP path supports");
  t->fbank = true;
  t->use_log_fbank = o.use_log_fbank;
  t->use_power = o.use_power;
  t->nceps = o.Dim();
  t->energy_col = !o.use_energy ? -1 : o.htk_compat ? o.num_bins : 0;      // feature-fbank.cc:102,120
  t->mel_col0 = (o.use_energy && !o.htk_compat) ? 1 : 0;
  t->dct.assign(1, 0.0f);
  t->lifter.assign(1, 1.0f);
}

static void ReadCmvnOptions(const std::string &path, CmvnOptions *c) {
  for (auto &kv : ReadConfigFile(path)) {
    const std::string &k = kv.first, &v = kv.second;
    if (k == "cmn-window") c->cmn_window = std::stoi(v);
    else if (k == "speaker-frames") c->speaker_frames = std::stoi(v);
    else if (k == "global-frames") c->global_frames = std::stoi(v);
    else if (k == "norm-means" || k == "norm-mean") c->normalize_mean = ParseBool(v, k);
    else if (k == "norm-vars") c->normalize_variance = ParseBool(v, k);
    else if (k == "skip-dims") { if (!v.empty()) Fail("online cmvn: --skip-dims is not supported"); }
    else Fail("Invalid option --" + k + " in config file " + path);
  }
  if (c->normalize_variance) Fail("online cmvn: --norm-vars=true is not supported by the HIP feature kernels");
}

static void ReadDiagGmm(const std::string &path, IvectorExtractor *ie) {
  KaldiReader r(path);
  std::string tok = r.ReadToken();
  if (tok != "<DiagGMMBegin>" && tok != "<DiagGMM>") Fail(path + ": Expected <DiagGMM>, got " + tok);
  tok = r.ReadToken();
  if (tok == "<GCONSTS>") {
    r.ReadVector(&ie->gconsts);
    r.ExpectToken("<WEIGHTS>");
  } else if (tok != "<WEIGHTS>") {
    Fail(path + ": DiagGmm::Read, expected <WEIGHTS> or <GCONSTS>, got " + tok);
  }
  r.ReadVector(&ie->weights);
  r.ExpectToken("<MEANS_INVVARS>");
  r.ReadMatrix(&ie->means_invvars);
  r.ExpectToken("<INV_VARS>");
  r.ReadMatrix(&ie->inv_vars);
  tok = r.ReadToken();
  if (tok != "<DiagGMMEnd>" && tok != "</DiagGMM>") Fail(path + ": Expected </DiagGMM>, got " + tok);
  // DiagGmm::ComputeGconsts (gmm/diag-gmm.cc:114-150): gconsts are always recomputed on read.
  int G = ie->means_invvars.rows, D = ie->means_invvars.cols;
  ie->gconsts.assign(G, 0.0f);
  float offset = (float)(-0.5 * 1.8378770664093454835606594728112 * D);  // M_LOG_2PI
  for (int g = 0; g < G; g++) {
    float gc = logf(ie->weights[g]) + offset;
    for (int d = 0; d < D; d++) {
      float iv = ie->inv_vars(g, d), miv = ie->means_invvars(g, d);
      // the reference's expression mixes double literals with float operands (evaluated in double)
      gc = (float)((double)gc + (0.5 * (double)logf(iv) - 0.5 * (double)miv * (double)miv / (double)iv));
    }
    if (std::isnan(gc)) Fail(path + ": not a number in gconst computation");
    if (std::isinf(gc) && gc > 0) gc = -gc;
    ie->gconsts[g] = gc;
  }
}

static void ReadIvectorExtractorFile(const std::string &path, IvectorExtractor *ie) {
  KaldiReader r(path);
  r.ExpectToken("<IvectorExtractor>");
  r.ExpectToken("<w>");
  MatD w;
  r.ReadMatrixD(&w);
  if (w.rows != 0) Fail(path + ": iVector extractors with iVector-dependent weights are not supported");
  r.ExpectToken("<w_vec>");
  std::vector<double> wv;
  r.ReadVectorD(&wv);
  r.ExpectToken("<M>");
  int n = r.ReadInt32();
  if (n <= 0) Fail(path + ": bad number of Gaussians");
  ie->M.resize(n);
  for (int i = 0; i < n; i++) r.ReadMatrixD(&ie->M[i]);
  r.ExpectToken("<SigmaInv>");
  ie->sigma_inv.resize(n);
  for (int i = 0; i < n; i++) {
    int dim;
    r.ReadSpMatrixD(&dim, &ie->sigma_inv[i]);
    if (dim != ie->M[i].rows) Fail(path + ": SigmaInv dim mismatch");
  }
  r.ExpectToken("<IvectorOffset>");
  ie->prior_offset = r.ReadDouble();
  r.ExpectToken("</IvectorExtractor>");
}

void IvectorExtractor::ComputeDerived() {
  // ivector-extractor.cc:205-218: U_g = M_g^T Sigma_g^{-1} M_g (packed), Sigma_inv_M_g = Sigma_g^{-1} M_g
  int G = num_gauss(), D = feat_dim(), I = ivector_dim();
  size_t usz = (size_t)I * (I + 1) / 2;
  U.assign((size_t)G * usz, 0.0);
  sigma_inv_M.assign((size_t)G * D * I, 0.0);
  std::vector<double> S((size_t)D * D);
  for (int g = 0; g < G; g++) {
    const std::vector<double> &p = sigma_inv[g];
    for (int r = 0, k = 0; r < D; r++)
      for (int c = 0; c <= r; c++, k++) S[(size_t)r * D + c] = S[(size_t)c * D + r] = p[k];
    double *sim = &sigma_inv_M[(size_t)g * D * I];
    const MatD &Mg = M[g];
    for (int r = 0; r < D; r++)
      for (int c = 0; c < D; c++) {
        double s = S[(size_t)r * D + c];
        if (s == 0.0) continue;
        const double *mrow = &Mg.d[(size_t)c * I];
        double *orow = &sim[(size_t)r * I];
        for (int i = 0; i < I; i++) orow[i] += s * mrow[i];
      }
    double *u = &U[(size_t)g * usz];
    for (int i = 0, k = 0; i < I; i++)
      for (int j = 0; j <= i; j++, k++) {
        double acc = 0;
        for (int d = 0; d < D; d++) acc += Mg.d[(size_t)d * I + i] * sim[(size_t)d * I + j];
        u[k] = acc;
      }
  }
}

static std::string DirName(const std::string &p) {
  size_t s = p.find_last_of('/');
  return s == std::string::npos ? "." : p.substr(0, s);
}

static void ReadKaldiMatrixFile(const std::string &path, MatF *m) { KaldiReader r(path); r.ReadMatrix(m); }
static void ReadKaldiMatrixFileD(const std::string &path, MatD *m) { KaldiReader r(path); r.ReadMatrixD(m); }

static void ReadIvectorConfig(const std::string &path, IvectorExtractor *ie, int base_dim) {
  std::string lda, gstats, cmvn_conf, splice_conf, ubm, extractor;
  for (auto &kv : ReadConfigFile(path)) {
    const std::string &k = kv.first, &v = kv.second;
    if (k == "lda-matrix") lda = v;
    else if (k == "global-cmvn-stats") gstats = v;
    else if (k == "cmvn-config") cmvn_conf = v;
    else if (k == "online-cmvn-iextractor") ie->online_cmvn_iextractor = ParseBool(v, k);
    else if (k == "splice-config") splice_conf = v;
    else if (k == "diag-ubm") ubm = v;
    else if (k == "ivector-extractor") extractor = v;
    else if (k == "ivector-period") ie->ivector_period = std::stoi(v);
    else if (k == "num-gselect") ie->num_gselect = std::stoi(v);
    else if (k == "min-post") ie->min_post = std::stof(v);
    else if (k == "posterior-scale") ie->posterior_scale = std::stof(v);
    else if (k == "max-count") ie->max_count = std::stof(v);
    else if (k == "num-cg-iters") ie->num_cg_iters = std::stoi(v);
    else if (k == "use-most-recent-ivector") ie->use_most_recent_ivector = ParseBool(v, k);
    else if (k == "greedy-ivector-extractor") ie->greedy = ParseBool(v, k);
    else if (k == "max-remembered-frames") ie->max_remembered_frames = std::stof(v);
    else Fail("Invalid option --" + k + " in config file " + path);
  }
  const char *note = " (note: this may be needed in the file supplied to --ivector-extractor-config)";
  if (lda.empty()) Fail(std::string("--lda-matrix option must be set") + note);
  if (gstats.empty()) Fail(std::string("--global-cmvn-stats option must be set") + note);
  if (cmvn_conf.empty()) Fail(std::string("--cmvn-config option must be set") + note);
  if (splice_conf.empty()) Fail(std::string("--splice-config option must be set") + note);
  if (ubm.empty()) Fail(std::string("--diag-ubm option must be set") + note);
  if (extractor.empty()) Fail(std::string("--ivector-extractor option must be set") + note);
  if (ie->greedy) ie->use_most_recent_ivector = true;
  ReadKaldiMatrixFile(lda, &ie->lda);
  ReadKaldiMatrixFileD(gstats, &ie->global_cmvn);
  ReadCmvnOptions(cmvn_conf, &ie->cmvn);
  for (auto &kv : ReadConfigFile(splice_conf)) {
    if (kv.first == "left-context") ie->splice_left = std::stoi(kv.second);
    else if (kv.first == "right-context") ie->splice_right = std::stoi(kv.second);
    else Fail("Invalid option --" + kv.first + " in config file " + splice_conf);
  }
  ReadDiagGmm(ubm, ie);
  ReadIvectorExtractorFile(extractor, ie);
  // OnlineIvectorExtractionInfo::Check (online-ivector-feature.cc:83-99)
  if (ie->global_cmvn.rows != 2) Fail("global_cmvn_stats must have 2 rows");
  int bdim = ie->global_cmvn.cols - 1, nsp = ie->splice_left + 1 + ie->splice_right;
  if (bdim != base_dim) Fail("iVector extractor: global CMVN stats dim " + std::to_string(bdim) + " != feature dim " + std::to_string(base_dim));
  if (ie->lda.cols != bdim * nsp && ie->lda.cols != bdim * nsp + 1) Fail("iVector extractor: LDA matrix has wrong number of columns");
  if (ie->lda.rows != ie->means_invvars.cols) Fail("iVector extractor: LDA rows != UBM dim");
  if (ie->means_invvars.cols != ie->M[0].rows) Fail("iVector extractor: UBM dim != extractor feature dim");
  if ((int)ie->M.size() != ie->means_invvars.rows) Fail("iVector extractor: #Gaussians mismatch between UBM and extractor");
  if (ie->ivector_period <= 0 || ie->num_gselect <= 0 || !(ie->min_post < 0.5f) ||
      !(ie->posterior_scale > 0.0f && ie->posterior_scale <= 1.0f))
    Fail("iVector extractor: invalid options");
  ie->ComputeDerived();
  ie->present = true;
}

void ReadFeatureConfig(const std::string &online_conf, FeatureConfig *fc) {
  std::string mfcc_conf, fbank_conf, ivec_conf, cmvn_conf, gstats;
  fc->conf_path = online_conf;
  for (auto &kv : ReadConfigFile(online_conf)) {
    const std::string &k = kv.first, &v = kv.second;
    if (k == "feature-type") fc->feature_type = v;
    else if (k == "mfcc-config") mfcc_conf = v;
    else if (k == "ivector-extraction-config") ivec_conf = v;
    else if (k == "cmvn-config") cmvn_conf = v;
    else if (k == "global-cmvn-stats") gstats = v;
    else if (k == "add-pitch") { if (ParseBool(v, k)) Fail("--add-pitch=true is not supported"); }
    else if (k == "fbank-config") fbank_conf = v;
    else if (k == "plp-config" || k == "online-pitch-config") {}
    // OnlineEndpointConfig (online-endpoint.h:159-186): kept as written; parsed by the first endpoint call, so that a model that
    // loaded before still loads whatever these lines say (Model::EndpointOpts)
    else if (k.compare(0, 9, "endpoint.") == 0) fc->endpoint_conf.emplace_back(k, v);
    else if (k.compare(0, 26, "ivector-silence-weighting.") == 0) {}
    // decodable / decoder options registered on the same parser (NnetSimpleLoopedComputationOptions, decodable-simple-looped.h:68-81;
    // LatticeFasterDecoderConfig + its det_opts, lattice-faster-decoder.h:67-85; the binaries' own --online, --do-endpointing,
    // --chunk-length ...): kept, and applied or refused by Model::Model -- never dropped
    else if (k == "frame-subsampling-factor" || k == "frames-per-chunk" || k == "acoustic-scale" ||
             k == "extra-left-context-initial" || k == "beam" || k == "max-active" || k == "min-active" ||
             k == "lattice-beam" || k == "beam-delta" || k == "prune-interval" || k == "hash-ratio" ||
             k == "determinize-lattice" || k == "minimize" || k == "phone-determinize" || k == "word-determinize" ||
             k == "max-mem" || k == "debug-computation" || k == "online" || k == "do-endpointing" || k == "chunk-length" ||
             k == "delta" || k == "num-threads-startup")
      fc->decoder_conf.emplace_back(k, v);
    else Fail("Invalid option --" + k + "=" + v + " in config file " + online_conf);
  }
  if (fc->feature_type != "mfcc" && fc->feature_type != "fbank") {
    if (fc->feature_type == "plp") Fail("feature type plp is not supported by the HIP path (supported: mfcc, fbank)");
    Fail("Invalid feature type: " + fc->feature_type + ". Supported feature types: mfcc, plp, fbank.");
  }
  // online-nnet2-feature-pipeline.cc:36-55: only the selected type's options are used; no config file means its defaults
  MfccOptions mo;
  if (!mfcc_conf.empty()) ReadMfccOptions(mfcc_conf, &mo);      // (read, and ignored, beside --feature-type=fbank too)
  if (fc->feature_type == "fbank") {
    FbankOptions fo;
    if (!fbank_conf.empty()) ReadFbankOptions(fbank_conf, &fo);
    BuildFbankTables(fo, &fc->mfcc);
  } else {
    BuildMfccTables(mo, &fc->mfcc);
  }
  const int feat_dim = fc->mfcc.nceps;
  fc->use_cmvn = !cmvn_conf.empty();
  if (fc->use_cmvn) {
    ReadCmvnOptions(cmvn_conf, &fc->cmvn);
    if (gstats.empty()) Fail("--global-cmvn-stats option is required  when --cmvn-config is specified.");
    ReadKaldiMatrixFileD(gstats, &fc->global_cmvn);
    if (fc->global_cmvn.rows != 2 || fc->global_cmvn.cols != feat_dim + 1) Fail("global cmvn stats have the wrong dimension");
  }
  if (!ivec_conf.empty()) ReadIvectorConfig(ivec_conf, &fc->ie, feat_dim);
}

// =============================================================================== transition model

void TransitionModel::Read(KaldiReader &r) {
  r.ExpectToken("<TransitionModel>");
  r.ExpectToken("<Topology>");
  // per topology entry: per state: (forward_pdf_class, self_loop_pdf_class, transitions (dst, prob))
  std::vector<std::vector<HmmState>> entries;
  std::vector<int32_t> phones, phone2idx;
  if (r.binary()) {
    r.ReadIntVector(&phones);
    r.ReadIntVector(&phone2idx);
    int sz = r.ReadInt32();
    bool is_hmm = true;
    if (sz == -1) { is_hmm = false; sz = r.ReadInt32(); }
    entries.resize(sz);
    for (int i = 0; i < sz; i++) {
      int ns = r.ReadInt32();
      entries[i].resize(ns);
      for (int j = 0; j < ns; j++) {
        entries[i][j].fwd = r.ReadInt32();
        entries[i][j].self = is_hmm ? entries[i][j].fwd : r.ReadInt32();
        int nt = r.ReadInt32();
        entries[i][j].trans.resize(nt);
        for (int k = 0; k < nt; k++) { entries[i][j].trans[k].first = r.ReadInt32(); entries[i][j].trans[k].second = r.ReadFloat(); }
      }
    }
    r.ExpectToken("</Topology>");
  } else {
    while (true) {
      std::string tok = r.ReadToken();
      if (tok == "</Topology>") break;
      if (tok != "<TopologyEntry>") Fail("Reading HmmTopology object, expected </Topology> or <TopologyEntry>, got " + tok);
      r.ExpectToken("<ForPhones>");
      std::vector<int> these;
      while (true) {
        std::string s = r.ReadToken();
        if (s == "</ForPhones>") break;
        these.push_back(std::stoi(s));
      }
      std::vector<HmmState> entry;
      tok = r.ReadToken();
      while (tok != "</TopologyEntry>") {
        if (tok != "<State>") Fail("Expected </TopologyEntry> or <State>, got instead " + tok);
        int state = r.ReadInt32();
        if (state != (int)entry.size()) Fail("States are expected to be in order from zero");
        HmmState hs;
        tok = r.ReadToken();
        if (tok == "<PdfClass>") { hs.fwd = hs.self = r.ReadInt32(); tok = r.ReadToken(); }
        else if (tok == "<ForwardPdfClass>") {
          hs.fwd = r.ReadInt32();
          r.ExpectToken("<SelfLoopPdfClass>");
          hs.self = r.ReadInt32();
          tok = r.ReadToken();
        }
        while (tok == "<Transition>") {
          int dst = r.ReadInt32();
          float p = r.ReadFloat();
          hs.trans.emplace_back(dst, p);
          tok = r.ReadToken();
        }
        if (tok != "</State>") Fail("Expected </State>, got instead " + tok);
        entry.push_back(hs);
        tok = r.ReadToken();
      }
      int idx = (int)entries.size();
      entries.push_back(entry);
      for (int p : these) {
        if ((int)phone2idx.size() <= p) phone2idx.resize(p + 1, -1);
        if (p <= 0 || phone2idx[p] != -1) Fail("bad phone in topology");
        phone2idx[p] = idx;
        phones.push_back(p);
      }
    }
  }
  std::string tok = r.ReadToken();
  if (tok != "<Triples>" && tok != "<Tuples>") Fail("TransitionModel: expected <Triples> or <Tuples>, got " + tok);
  const bool has_self = (tok == "<Tuples>");
  int n = r.ReadInt32();
  std::vector<Tuple> tp(n);
  for (int i = 0; i < n; i++) {
    tp[i].phone = r.ReadInt32();
    tp[i].hmm_state = r.ReadInt32();
    tp[i].fwd = r.ReadInt32();
    tp[i].self = has_self ? r.ReadInt32() : tp[i].fwd;
  }
  tok = r.ReadToken();
  if (tok != "</Triples>" && tok != "</Tuples>") Fail("TransitionModel: expected </Triples> or </Tuples>");
  // ComputeDerived (transition-model.cc:144-177)
  id2pdf.assign(1, 0);
  id2phone.assign(1, 0);
  id2hmm_state.assign(1, 0);
  id2self_loop.assign(1, 0);
  std::vector<int> self_loop_of(1, 0);      // per transition-id: the self-loop transition-id of its transition-state (0 = none)
  topo_entries = entries;
  phone2entry = phone2idx;
  tuples = tp;
  tstate_first_tid.assign(1, 0);
  id2tstate.assign(1, 0);
  num_pdfs = 0;
  for (int ts = 0; ts < n; ts++) {
    const Tuple &t = tp[ts];
    if (t.phone <= 0 || t.phone >= (int)phone2idx.size() || phone2idx[t.phone] < 0) Fail("TransitionModel: phone without topology");
    const auto &entry = entries[phone2idx[t.phone]];
    if (t.hmm_state < 0 || t.hmm_state >= (int)entry.size()) Fail("TransitionModel: bad hmm-state");
    const HmmState &hs = entry[t.hmm_state];
    num_pdfs = std::max(num_pdfs, 1 + std::max(t.fwd, t.self));
    const int first_tid = (int)id2pdf.size();
    tstate_first_tid.push_back(first_tid);
    int sl_tid = 0;
    for (size_t k = 0; k < hs.trans.size(); k++) {
      bool self_loop = (hs.trans[k].first == t.hmm_state);
      if (self_loop && sl_tid == 0) sl_tid = first_tid + (int)k;       // SelfLoopOf (transition-model.cc:360-373)
      id2pdf.push_back(self_loop ? t.self : t.fwd);
      id2phone.push_back(t.phone);
      id2hmm_state.push_back(t.hmm_state);
      id2self_loop.push_back(self_loop ? 1 : 0);
      id2tstate.push_back(ts + 1);
    }
    for (size_t k = 0; k < hs.trans.size(); k++) self_loop_of.push_back(sl_tid);
  }
  self_loop_of_id = self_loop_of;
  r.ExpectToken("<LogProbs>");
  std::vector<float> lp;
  r.ReadVector(&lp);
  if (lp.size() != id2pdf.size()) Fail("TransitionModel: <LogProbs> size does not match the number of transition-ids");
  log_prob = lp;
  // ComputeDerivedOfProbs (transition-model.cc:375-392)
  non_self_loop_log_prob.assign(lp.size(), 0.0f);
  for (size_t tid = 1; tid < lp.size(); tid++) {
    if (self_loop_of[tid] == 0) continue;
    float p = 1.0f - expf(lp[self_loop_of[tid]]);
    if (p <= 0.0f) p = 1.0e-10f;
    non_self_loop_log_prob[tid] = logf(p);
  }
  r.ExpectToken("</LogProbs>");
  r.ExpectToken("</TransitionModel>");
}

int TransitionModel::TupleToTransitionState(int phone, int hmm_state, int fwd, int self) const {
  // transition-model.cc:179-196: binary search in the sorted tuple table
  size_t lo = 0, hi = tuples.size();
  auto less = [](const Tuple &a, int p, int h, int f, int s) {
    if (a.phone != p) return a.phone < p;
    if (a.hmm_state != h) return a.hmm_state < h;
    if (a.fwd != f) return a.fwd < f;
    return a.self < s;
  };
  while (lo < hi) { const size_t mid = (lo + hi) / 2; if (less(tuples[mid], phone, hmm_state, fwd, self)) lo = mid + 1; else hi = mid; }
  if (lo < tuples.size() && tuples[lo].phone == phone && tuples[lo].hmm_state == hmm_state && tuples[lo].fwd == fwd && tuples[lo].self == self)
    return (int)lo + 1;
  return 0;
}

int TransitionModel::NumPdfClasses(int phone) const {
  // hmm-topology.cc:275-285: 1 + the largest pdf class of the phone's entry
  if (phone <= 0 || phone >= (int)phone2entry.size() || phone2entry[phone] < 0) Fail("TransitionModel: phone " + std::to_string(phone) + " has no topology");
  int mx = -1;
  for (const HmmState &h : topo_entries[phone2entry[phone]]) mx = std::max(mx, std::max(h.fwd, h.self));
  return mx + 1;
}

// =============================================================================== nnet3 parsing

static const std::set<std::string> kIntVectorFields = {"<TimeOffsets>", "<ColumnMap>", "<Sizes>"};

static Component ReadComponent(KaldiReader &r) {
  Component c;
  std::string open = r.ReadToken();
  if (open.size() < 3 || open[0] != '<' || open.back() != '>') Fail(r.name() + ": expected a component opening tag, got " + open.substr(0, 40));
  c.type = open.substr(1, open.size() - 2);
  std::string close = "</" + c.type + ">";
  while (true) {
    std::string tok = r.ReadToken();
    if (tok == close) break;
    if (tok.empty() || tok[0] != '<') Fail(r.name() + ": malformed component " + c.type + " near " + tok.substr(0, 40));
    if (kIntVectorFields.count(tok)) { r.ReadIntVector(&c.iv[tok]); continue; }
    if (c.type == "TimeHeightConvolutionComponent") {
      // ConvolutionModel::Read (convolution.cc:252-280): <Offsets> is a vector of (time, height) pairs, kept flat
      if (tok == "<Offsets>") { r.ReadIntPairVector(&c.iv[tok]); continue; }
      if (tok == "<RequiredTimeOffsets>") { r.ReadIntVector(&c.iv[tok]); continue; }
    }
    c.b[tok] = true;   // present (bare flag unless values follow)
    while (true) {
      int ch = r.PeekChar();
      if (ch < 0) Fail(r.name() + ": unexpected EOF in component " + c.type);
      if (ch == '<') break;
      if (r.binary()) {
        if (ch == 4 || ch == 8) { double fv; int64_t iv; r.ReadBasicAny(&fv, &iv); c.f[tok].push_back(fv); c.i[tok].push_back(iv); continue; }
        std::string head = r.PeekToken();
        if (head == "FM" || head == "DM" || head == "CM" || head == "CM2" || head == "CM3") { r.ReadMatrix(&c.m[tok]); continue; }
        if (head == "FV" || head == "DV") { r.ReadVector(&c.v[tok]); continue; }
        if (ch == 'T' || ch == 'F') { bool bv = r.ReadBool(); c.f[tok].push_back(bv ? 1.0 : 0.0); c.i[tok].push_back(bv); continue; }
        Fail(r.name() + ": cannot parse field " + tok + " of component " + c.type);
      } else {
        if (ch == '[') {
          // vector or matrix: decide by row count
          MatF m;
          r.ReadMatrix(&m);
          // (<Params> is a matrix in a LinearComponent or an LstmNonlinearityComponent, a vector in the per-element scales)
          const bool scales = c.type == "PerElementScaleComponent" || c.type == "NaturalGradientPerElementScaleComponent";
          if (m.rows <= 1 && tok != "<LinearParams>" && (tok != "<Params>" || scales)) c.v[tok] = m.d;
          else c.m[tok] = m;
          continue;
        }
        if (ch == 'T' || ch == 'F') {
          std::string t = r.PeekToken();
          if (t == "T" || t == "F") { bool bv = r.ReadBool(); c.f[tok].push_back(bv ? 1.0 : 0.0); c.i[tok].push_back(bv); continue; }
        }
        { double fv; int64_t iv; r.ReadBasicAny(&fv, &iv); c.f[tok].push_back(fv); c.i[tok].push_back(iv); }
      }
    }
  }
  return c;
}

// The <ConvolutionModel> of a TimeHeightConvolutionComponent with what ConvolutionModel::Check(false, true) (convolution.cc:
// 130-209) and TimeHeightConvolutionComponent::Check ask of it and of the parameters.
ConvGeom ReadConvGeom(const Component &c, const std::string &name) {
  const std::string what = "nnet3: TimeHeightConvolutionComponent '" + name + "': ";
  for (const char *k : {"<NumFiltersIn>", "<NumFiltersOut>", "<HeightIn>", "<HeightOut>", "<HeightSubsampleOut>"})
    if (!c.i.count(k)) Fail(what + "no " + k);
  ConvGeom g;
  g.filters_in = c.Int("<NumFiltersIn>"); g.filters_out = c.Int("<NumFiltersOut>");
  g.height_in = c.Int("<HeightIn>"); g.height_out = c.Int("<HeightOut>"); g.height_sub = c.Int("<HeightSubsampleOut>");
  auto oit = c.iv.find("<Offsets>"), rit = c.iv.find("<RequiredTimeOffsets>");
  if (oit == c.iv.end() || rit == c.iv.end()) Fail(what + "no <Offsets> or <RequiredTimeOffsets>");
  for (size_t i = 0; i + 1 < oit->second.size(); i += 2) g.offsets.emplace_back(oit->second[i], oit->second[i + 1]);
  const std::set<int> required(rit->second.begin(), rit->second.end());
  if (g.filters_in <= 0 || g.filters_out <= 0 || g.height_in <= 0 || g.height_out <= 0 || g.height_sub <= 0 || g.offsets.empty() ||
      required.empty())
    Fail(what + "Convolution model fails basic check.");
  if (g.filters_in > 4096 || g.filters_out > 4096 || g.height_in > 4096 || g.height_out > 4096 || g.height_sub > 4096 || g.offsets.size() > 4096)
    Fail(what + "a dimension above 4096 is not supported by the HIP convolution kernel");
  for (size_t i = 0; i + 1 < g.offsets.size(); i++)
    if (!(g.offsets[i] < g.offsets[i + 1])) Fail(what + "the (time, height) offsets are not sorted and unique");
  std::set<int> all;
  for (auto &o : g.offsets) {
    if (std::abs(o.first) > 4096 || std::abs(o.second) > 4096) Fail(what + "an offset beyond +-4096 is not supported");
    all.insert(o.first);
  }
  for (int t : required)
    if (!all.count(t)) Fail(what + "Required time offsets not a subset of all_time_offsets.");
  std::vector<char> used(g.offsets.size(), 0);
  for (int h = 0; h < g.height_out; h++) {
    bool some = false;
    for (size_t i = 0; i < g.offsets.size(); i++) {
      const int h_in = h * g.height_sub + g.offsets[i].second;
      if (h_in < 0 || h_in >= g.height_in) continue;
      used[i] = 1;
      if (required.count(g.offsets[i].first)) some = true;
    }
    if (!some) Fail(what + "for the " + std::to_string(h) + "'th output height, no input is available, if only required time-indexes are available.");
  }
  for (size_t i = 0; i < used.size(); i++)
    if (!used[i])
      Fail(what + "(time,height) offset (" + std::to_string(g.offsets[i].first) + "," + std::to_string(g.offsets[i].second) + ") of this computation is never used.");
  // Zero padding in time: a frame whose optional offsets fall outside the chunk's input gets zeros for them, so the result
  // depends on where the chunk boundaries lie.  Never approximated.
  if (required.size() != all.size())
    Fail(what + "its required time offsets are a proper subset of its time offsets (zero padding in time, whose result depends on the frames "
                "a chunk holds): not supported by the HIP acoustic-model kernels");
  g.time_offsets.assign(all.begin(), all.end());
  auto wit = c.m.find("<LinearParams>");
  auto bit = c.v.find("<BiasParams>");
  if (wit == c.m.end() || bit == c.v.end()) Fail(what + "no <LinearParams> or <BiasParams>");
  if (wit->second.rows != g.filters_out || wit->second.cols != g.K())
    Fail(what + "<LinearParams> is " + std::to_string(wit->second.rows) + " x " + std::to_string(wit->second.cols) + ", the model needs " +
         std::to_string(g.filters_out) + " x " + std::to_string(g.K()));
  if ((int)bit->second.size() != g.filters_out) Fail(what + "<BiasParams> has " + std::to_string(bit->second.size()) + " elements, not " + std::to_string(g.filters_out));
  return g;
}

// The fields of a RestrictedAttentionComponent (Write, nnet-attention-component.cc:442-471; the statistics behind <KeyScale> are
// read and dropped) with what RestrictedAttentionComponent::Check() (:277-289) asks of them.
AttentionGeom ReadAttentionGeom(const Component &c, const std::string &name, const std::string &node) {
  const std::string what = "nnet3: RestrictedAttentionComponent '" + name + "'" + (node.empty() ? std::string() : " (node " + node + ")") + ": ";
  for (const char *k : {"<NumHeads>", "<KeyDim>", "<ValueDim>", "<NumLeftInputs>", "<NumRightInputs>", "<TimeStride>", "<NumLeftInputsRequired>",
                        "<NumRightInputsRequired>", "<OutputContext>"})
    if (!c.i.count(k) || c.i.at(k).empty()) Fail(what + "no " + k);
  if (!c.f.count("<KeyScale>") || c.f.at("<KeyScale>").empty()) Fail(what + "no <KeyScale>");
  AttentionGeom g;
  g.heads = c.Int("<NumHeads>"); g.key_dim = c.Int("<KeyDim>"); g.value_dim = c.Int("<ValueDim>");
  g.left = c.Int("<NumLeftInputs>"); g.right = c.Int("<NumRightInputs>"); g.stride = c.Int("<TimeStride>");
  g.output_context = c.Int("<OutputContext>") != 0;
  g.key_scale = (float)c.f.at("<KeyScale>")[0];
  const int left_req = c.Int("<NumLeftInputsRequired>"), right_req = c.Int("<NumRightInputsRequired>");
  const double stats_count = c.f.count("<StatsCount>") && !c.f.at("<StatsCount>").empty() ? c.f.at("<StatsCount>")[0] : 0.0;
  auto check = [&](bool ok, const char *clause) { if (!ok) Fail(what + "Check() fails: " + clause); };
  check(g.heads > 0 && g.key_dim > 0 && g.value_dim > 0, "num_heads_ > 0 && key_dim_ > 0 && value_dim_ > 0");
  check(g.left >= 0 && g.right >= 0 && g.left + g.right > 0,
        "num_left_inputs_ >= 0 && num_right_inputs_ >= 0 && (num_left_inputs_ + num_right_inputs_) > 0");
  check(g.stride > 0, "time_stride_ > 0");
  check(left_req >= 0 && left_req <= g.left, "num_left_inputs_required_ >= 0 && num_left_inputs_required_ <= num_left_inputs_");
  check(right_req >= 0 && right_req <= g.right, "num_right_inputs_required_ >= 0 && num_right_inputs_required_ <= num_right_inputs_");
  check(g.key_scale > 0.0f && g.key_scale <= 1.0f, "key_scale_ > 0.0 && key_scale_ <= 1.0");
  check(stats_count >= 0.0, "stats_count_ >= 0.0");
  // Zero padding in time: a frame whose optional inputs fall outside the chunk's input attends to zero rows in their place, so the
  // result depends on where the chunk boundaries lie.  Never approximated.
  if (left_req < g.left)
    Fail(what + "num-left-inputs-required " + std::to_string(left_req) + " is smaller than num-left-inputs " + std::to_string(g.left) +
         " (zero padding in time, whose result depends on the frames a chunk holds): not supported by the HIP acoustic-model kernels");
  if (right_req < g.right)
    Fail(what + "num-right-inputs-required " + std::to_string(right_req) + " is smaller than num-right-inputs " + std::to_string(g.right) +
         " (zero padding in time, whose result depends on the frames a chunk holds): not supported by the HIP acoustic-model kernels");
  return g;
}

// ---- descriptor parser (nnet3/nnet-descriptor.cc grammar subset) ----
namespace {
struct DescParser {
  const std::string &s;
  size_t p = 0;
  const Nnet &net;
  const std::vector<int> &node_dims;
  DescParser(const std::string &str, const Nnet &n, const std::vector<int> &dims) : s(str), net(n), node_dims(dims) {}
  void Ws() { while (p < s.size() && std::isspace((unsigned char)s[p])) p++; }
  std::string Ident() {
    Ws();
    size_t b = p;
    while (p < s.size() && (std::isalnum((unsigned char)s[p]) || s[p] == '_' || s[p] == '-' || s[p] == '.')) p++;
    return s.substr(b, p - b);
  }
  void Expect(char c) {
    Ws();
    if (p >= s.size() || s[p] != c) Fail("nnet3 descriptor parse error in '" + s + "' at " + std::to_string(p) + ": expected '" + c + "'");
    p++;
  }
  double Number() {
    Ws();
    const char *b = s.c_str() + p;
    char *e;
    double v = std::strtod(b, &e);
    if (e == b) Fail("nnet3 descriptor parse error in '" + s + "': expected number");
    p += e - b;
    return v;
  }
  std::vector<DescPart> Parse() {
    size_t save = p;
    std::string id = Ident();
    Ws();
    if (p < s.size() && s[p] == '(') {
      p++;
      std::vector<DescPart> out;
      if (id == "Append") {
        while (true) {
          auto sub = Parse();
          out.insert(out.end(), sub.begin(), sub.end());
          Ws();
          if (p < s.size() && s[p] == ',') { p++; continue; }
          break;
        }
      } else if (id == "Sum") {
        out = Parse();
        while (true) {
          Ws();
          if (p < s.size() && s[p] == ',') {
            p++;
            auto b = Parse();
            if (b.size() != out.size()) Fail("nnet3 descriptor: Sum() of differently structured Appends is not supported: " + s);
            for (size_t i = 0; i < out.size(); i++) {
              if (b[i].dim != out[i].dim) Fail("nnet3 descriptor: Sum() dimension mismatch: " + s);
              out[i].terms.insert(out[i].terms.end(), b[i].terms.begin(), b[i].terms.end());
            }
            continue;
          }
          break;
        }
      } else if (id == "Offset") {
        out = Parse();
        Expect(',');
        int t = (int)Number();
        Ws();
        if (p < s.size() && s[p] == ',') { p++; if ((int)Number() != 0) Fail("nnet3 descriptor: x-offsets are not supported: " + s); }
        for (auto &pt : out) for (auto &tm : pt.terms) if (!tm.const_t) tm.offset += t;
      } else if (id == "Scale") {
        float sc = (float)Number();
        Expect(',');
        out = Parse();
        for (auto &pt : out) for (auto &tm : pt.terms) tm.scale *= sc;
      } else if (id == "ReplaceIndex") {
        out = Parse();
        Expect(',');
        std::string var = Ident();
        Expect(',');
        int val = (int)Number();
        if (var != "t" || val != 0) Fail("nnet3 descriptor: only ReplaceIndex(x, t, 0) is supported: " + s);
        for (auto &pt : out) for (auto &tm : pt.terms) { tm.const_t = true; tm.offset = 0; }
      } else if (id == "IfDefined") {
        out = Parse();
        for (auto &pt : out) for (auto &tm : pt.terms) tm.optional = true;
      } else if (id == "Const") {
        // Const(value, dim): a term without a node; FindBlocks accepts it only as the (1 - z_t) of a composed GRU block
        DescPart part;
        DescTerm t;
        t.konst = true;
        t.scale = (float)Number();
        Expect(',');
        part.dim = (int)Number();
        if (part.dim <= 0) Fail("nnet3 descriptor: Const() with a dim of " + std::to_string(part.dim) + ": " + s);
        part.terms.push_back(t);
        out.push_back(part);
      } else {
        Fail("nnet3 descriptor: unsupported expression '" + id + "' in: " + s);
      }
      Expect(')');
      return out;
    }
    if (id.empty()) { p = save; Fail("nnet3 descriptor parse error in '" + s + "'"); }
    int n = net.FindNode(id);
    if (n < 0) Fail("nnet3 descriptor: unknown node '" + id + "' in: " + s);
    DescPart part;
    DescTerm t;
    t.node = n;
    part.terms.push_back(t);
    part.dim = node_dims[n];
    return {part};
  }
};

std::map<std::string, std::string> ParseConfigLine(const std::string &line, std::string *first) {
  // "component-node name=x component=y input=Append(a, b)" -> key/value; values run until the next " key=".
  std::map<std::string, std::string> kv;
  std::istringstream is(line);
  is >> *first;
  std::string rest;
  std::getline(is, rest);
  size_t i = 0;
  std::vector<std::pair<size_t, size_t>> keys;  // (key start, '=' pos)
  while (i < rest.size()) {
    if (std::isspace((unsigned char)rest[i])) { i++; continue; }
    size_t b = i;
    while (i < rest.size() && (std::isalnum((unsigned char)rest[i]) || rest[i] == '-' || rest[i] == '_')) i++;
    if (i < rest.size() && rest[i] == '=' && i > b && (b == 0 || std::isspace((unsigned char)rest[b - 1]))) {
      keys.emplace_back(b, i);
    }
    while (i < rest.size() && !std::isspace((unsigned char)rest[i])) i++;
  }
  for (size_t k = 0; k < keys.size(); k++) {
    size_t vb = keys[k].second + 1, ve = (k + 1 < keys.size()) ? keys[k + 1].first : rest.size();
    std::string v = rest.substr(vb, ve - vb);
    while (!v.empty() && std::isspace((unsigned char)v.back())) v.pop_back();
    kv[rest.substr(keys[k].first, keys[k].second - keys[k].first)] = v;
  }
  return kv;
}

int ComponentOutputDim(const Component &c, const std::string &name) {
  auto rows = [&](const char *k) -> int { auto it = c.m.find(k); return it == c.m.end() ? -1 : it->second.rows; };
  if (c.type == "AffineComponent" || c.type == "NaturalGradientAffineComponent" || c.type == "FixedAffineComponent" ||
      c.type == "TdnnComponent")
    return rows("<LinearParams>");
  if (c.type == "LinearComponent") return rows("<Params>");
  if (c.type == "LstmNonlinearityComponent") {      // (nnet-combined-component.cc:973-977: [c | m])
    auto it = c.m.find("<Params>");
    if (it == c.m.end() || it->second.rows != 3 || it->second.cols <= 0) Fail("nnet3: LstmNonlinearityComponent '" + name + "' needs a 3-row <Params> matrix");
    return 2 * it->second.cols;
  }
  if (c.type == "OutputGruNonlinearityComponent" || c.type == "GruNonlinearityComponent") {      // (nnet-combined-component.h: [h | c])
    if (!c.i.count("<CellDim>") || c.Int("<CellDim>") <= 0) Fail("nnet3: " + c.type + " '" + name + "' has no <CellDim>");
    if (c.type == "OutputGruNonlinearityComponent" && (!c.v.count("<w_h>") || (int)c.v.at("<w_h>").size() != c.Int("<CellDim>")))
      Fail("nnet3: OutputGruNonlinearityComponent '" + name + "' needs a <w_h> vector of <CellDim> elements");
    return 2 * c.Int("<CellDim>");
  }
  if ((c.type == "DropoutMaskComponent" || c.type == "ElementwiseProductComponent") && c.i.count("<OutputDim>")) return c.Int("<OutputDim>");
  if (c.type == "TimeHeightConvolutionComponent") { const ConvGeom g = ReadConvGeom(c, name); return g.filters_out * g.height_out; }
  if (c.type == "RestrictedAttentionComponent") return ReadAttentionGeom(c, name).OutDim();
  if (c.type == "PermuteComponent") {
    auto it = c.iv.find("<ColumnMap>");
    if (it == c.iv.end() || it->second.empty()) Fail("nnet3: PermuteComponent '" + name + "' has no <ColumnMap>");
    return (int)it->second.size();
  }
  if (c.type == "NormalizeComponent") {
    int d = c.i.count("<InputDim>") ? c.Int("<InputDim>") : c.Int("<Dim>");
    bool add = c.f.count("<AddLogStddev>") && c.f.at("<AddLogStddev>")[0] != 0.0;
    return d + (add ? 1 : 0);
  }
  if (c.i.count("<Dim>")) return c.Int("<Dim>");
  if (c.type == "PerElementScaleComponent" || c.type == "NaturalGradientPerElementScaleComponent" || c.type == "FixedScaleComponent") {
    auto it = c.v.find(c.type == "FixedScaleComponent" ? "<Scales>" : "<Params>");
    if (it != c.v.end()) return (int)it->second.size();
  }
  if (c.type == "PerElementOffsetComponent") { auto it = c.v.find("<Offsets>"); if (it != c.v.end()) return (int)it->second.size(); }
  if (c.type == "FixedBiasComponent") { auto it = c.v.find("<Bias>"); if (it != c.v.end()) return (int)it->second.size(); }
  if (c.type == "ScaleAndOffsetComponent") { auto it = c.v.find("<Scales>"); if (it != c.v.end()) return (int)it->second.size(); }
  Fail("nnet3: cannot determine the output dimension of component '" + name + "' of type " + c.type);
}
}  // namespace

int Nnet::FindNode(const std::string &name) const {
  for (size_t i = 0; i < nodes.size(); i++) if (nodes[i].name == name) return (int)i;
  return -1;
}

void ReadNnetComponents(KaldiReader &r, std::vector<std::string> *names, std::vector<Component> *comps) {
  r.ExpectToken("<NumComponents>");
  int nc = r.ReadInt32();
  if (nc < 0 || nc >= 100000) Fail("bad <NumComponents>");
  names->resize(nc);
  comps->resize(nc);
  for (int c = 0; c < nc; c++) {
    r.ExpectToken("<ComponentName>");
    (*names)[c] = r.ReadToken();
    (*comps)[c] = ReadComponent(r);
  }
  r.ExpectToken("</Nnet3>");
}

namespace {
void CheckRecurrence(const Nnet &net);
std::string AttentionInputRefusal(const std::string &node, bool ivector) {
  if (ivector) return "nnet3: attention node " + node + " reads the iVector input directly: not supported";
  return "nnet3: attention node " + node + " reads a Sum(), a Scale() or an Append() of several parts directly: its input must be one node or an Offset() of one";
}
}  // namespace

void Nnet::Read(KaldiReader &r, int frames_per_chunk, int extra_left_context_initial, int frame_subsampling_factor) {
  r.ExpectToken("<Nnet3>");
  std::string line = r.ReadLine();
  if (!line.empty() && line.find_first_not_of(" \t") != std::string::npos) Fail("Expected newline in config file, got " + line);
  std::vector<std::string> cfg;
  while (true) {
    if (r.RawEof()) Fail(r.name() + ": EOF inside <Nnet3> config section");
    line = r.ReadLine();
    if (line.empty()) break;
    cfg.push_back(line);
  }
  ReadNnetComponents(r, &component_names, &components);
  for (size_t c = 0; c < components.size(); c++)      // (checked before the set-up walks the network with their offsets)
    if (components[c].type == "TimeHeightConvolutionComponent") (void)ReadConvGeom(components[c], component_names[c]);
  // (a RestrictedAttentionComponent too; its refusal names the node that runs it, where the config lines parse)
  {
    std::vector<std::string> node_of(components.size());
    for (auto &l : cfg) {
      std::string first;
      auto kv = ParseConfigLine(l, &first);
      if (first != "component-node") continue;
      auto it = std::find(component_names.begin(), component_names.end(), kv["component"]);
      if (it != component_names.end() && node_of[it - component_names.begin()].empty()) node_of[it - component_names.begin()] = kv["name"];
    }
    for (size_t c = 0; c < components.size(); c++)
      if (components[c].type == "RestrictedAttentionComponent") (void)ReadAttentionGeom(components[c], component_names[c], node_of[c]);
  }
  // The network as written, and its cycles: a recurrence that is not a fast-lstm(p) or fast-(norm-)opgru block is refused here, with its node and the
  // reason, before the set-up below walks the network.  (Lines this parser does not take may belong to orphan nodes the set-up
  // drops: then the check waits for Compile, which sees the network the set-up leaves.)
  bool parsed = true;
  try { ParseNodes(cfg); } catch (const Error &) { parsed = false; }
  if (parsed) CheckRecurrence(*this);
  if (parsed) {
    // what an attention node may read: one node or an Offset() of one, not the iVector (refused here, with the node, before the
    // set-up walks a network it would take for something else)
    const int iv = FindNode("ivector");
    for (const NnetNode &nd : nodes) {
      if (nd.kind != NnetNode::kComponent || components[nd.component].type != "RestrictedAttentionComponent") continue;
      if (nd.input.parts.size() != 1 || nd.input.parts[0].terms.size() != 1 || nd.input.parts[0].terms[0].scale != 1.0f) Fail(AttentionInputRefusal(nd.name, false));
      if (nd.input.parts[0].terms[0].const_t || nd.input.parts[0].terms[0].node == iv) Fail(AttentionInputRefusal(nd.name, true));
    }
  }
  {
    // CollapseModel + the rand() calls of the reference's set-up (nnet3_setup.h); RS_NO_COLLAPSE=1 keeps the layers as
    // written (A/B of the rounding difference; the rand() count is that of the reference either way)
    std::vector<std::string> names = component_names;
    std::vector<Component> comps = components;
    const char *e = TuneEnv("RS_NO_COLLAPSE");
    const bool keep_layers = e && e[0] == '1';
    Nnet3SetupResult su = Nnet3Setup(cfg, keep_layers ? &names : &component_names, keep_layers ? &comps : &components, frames_per_chunk,
                                     extra_left_context_initial, frame_subsampling_factor);
    setup_rand_calls = su.rand_calls;
    setup_rand_certain = su.rand_calls_certain;
    setup_rand_uncertain_why = su.uncertain_why;
    if (!keep_layers) cfg = su.config;
  }
  ParseNodes(cfg);
}

void Nnet::ParseNodes(const std::vector<std::string> &cfg) {
  nodes.clear();
  // first pass: create nodes (names + dims), second pass: descriptors
  std::vector<std::map<std::string, std::string>> kvs;
  std::vector<std::string> firsts;
  for (auto &l : cfg) {
    std::string first;
    auto kv = ParseConfigLine(l, &first);
    if (first == "component") continue;   // "component name=... type=..." lines do not occur in written models
    NnetNode n;
    n.name = kv["name"];
    if (first == "input-node") { n.kind = NnetNode::kInput; n.dim = std::stoi(kv["dim"]); }
    else if (first == "component-node") {
      n.kind = NnetNode::kComponent;
      auto it = std::find(component_names.begin(), component_names.end(), kv["component"]);
      if (it == component_names.end()) Fail("nnet3: component-node " + n.name + " refers to unknown component " + kv["component"]);
      n.component = (int)(it - component_names.begin());
      n.dim = ComponentOutputDim(components[n.component], kv["component"]);
    } else if (first == "output-node") n.kind = NnetNode::kOutput;
    else if (first == "dim-range-node") { n.kind = NnetNode::kDimRange; n.dim = std::stoi(kv["dim"]); n.range_offset = std::stoi(kv["dim-offset"]); }
    else Fail("nnet3: unsupported config line: " + l);
    nodes.push_back(n);
    kvs.push_back(kv);
    firsts.push_back(first);
  }
  // resolve descriptors; dims of output nodes depend on their inputs, so iterate until stable
  std::vector<int> dims(nodes.size());
  for (size_t i = 0; i < nodes.size(); i++) dims[i] = nodes[i].dim;
  for (size_t i = 0; i < nodes.size(); i++) {
    NnetNode &n = nodes[i];
    if (n.kind == NnetNode::kDimRange) {
      n.range_node = FindNode(kvs[i]["input-node"]);
      if (n.range_node < 0) Fail("nnet3: dim-range-node " + n.name + " has unknown input-node");
    }
  }
  for (size_t i = 0; i < nodes.size(); i++) {
    NnetNode &n = nodes[i];
    if (n.kind != NnetNode::kComponent && n.kind != NnetNode::kOutput) continue;
    DescParser dp(kvs[i]["input"], *this, dims);
    n.input.parts = dp.Parse();
    dp.Ws();
    if (dp.p != dp.s.size()) Fail("nnet3: trailing characters in descriptor: " + dp.s);
    n.input.dim = 0;
    for (auto &p : n.input.parts) n.input.dim += p.dim;
    if (n.kind == NnetNode::kOutput) { n.dim = n.input.dim; dims[i] = n.dim; }
  }
  int in = FindNode("input"), iv = FindNode("ivector"), out = FindNode("output");
  if (in < 0 || nodes[in].kind != NnetNode::kInput) Fail("nnet3: no input-node named 'input'");
  if (out < 0 || nodes[out].kind != NnetNode::kOutput) Fail("nnet3: no output-node named 'output'");
  input_dim = nodes[in].dim;
  ivector_dim = iv >= 0 ? nodes[iv].dim : 0;
  output_dim = nodes[out].dim;
}

// =============================================================================== nnet3 compile

namespace {
bool IsAffineLike(const std::string &t) {
  return t == "AffineComponent" || t == "NaturalGradientAffineComponent" || t == "FixedAffineComponent" ||
         t == "LinearComponent" || t == "TdnnComponent";
}
bool IsIdentity(const Component &c) {
  return c.type == "NoOpComponent" || c.type == "DropoutComponent" || c.type == "GeneralDropoutComponent" ||
         c.type == "SpecAugmentTimeMaskComponent" || c.type == "ClipGradientComponent";
}
// BackpropTruncationComponent::Propagate (nnet-general-component.cc:1094-1102): out = in, then Scale(scale_) unless it is 1
float TruncationScale(const Component &c) {
  auto it = c.f.find("<Scale>");
  return it == c.f.end() || it->second.empty() ? 1.0f : (float)it->second[0];
}

// A ScaleAndOffsetComponent's two vectors as PropagateInternal applies them (nnet-simple-component.cc:2474-2485): the scales through
// cu::EnsureNonzero with the component's epsilon 1e-4 (|s| < 1e-4 becomes +-1e-4 with the sign of s, +1e-4 at 0), the offsets as read
void ScaleAndOffsetVectors(const Component &c, const std::string &name, std::vector<float> *scales, std::vector<float> *offsets) {
  auto sit = c.v.find("<Scales>"), oit = c.v.find("<Offsets>");
  if (!c.i.count("<Dim>") || sit == c.v.end() || oit == c.v.end() || sit->second.empty() || sit->second.size() != oit->second.size() ||
      c.Int("<Dim>") <= 0 || c.Int("<Dim>") % (int)sit->second.size() != 0)
    Fail("nnet3: ScaleAndOffsetComponent '" + name + "' needs a <Dim> that is a multiple of the length of its <Scales> and <Offsets> vectors");
  const float eps = 1.0e-4f;
  *scales = sit->second;
  for (float &x : *scales)
    if (!(x <= -eps || x >= eps)) x = x >= 0.0f ? eps : -eps;
  *offsets = oit->second;
}

// Elementwise component -> stages (empty = identity).  false if the type is not elementwise.
bool EltStagesFor(const Component &c, const std::string &name, std::vector<EltStage> *st) {
  st->clear();
  if (IsIdentity(c)) return true;
  if (c.type == "BackpropTruncationComponent") {
    const float scale = TruncationScale(c);
    if (scale != 1.0f) { EltStage s; s.kind = EltStage::kScale; s.alpha = scale; st->push_back(s); }
    return true;
  }
  if (c.type == "RectifiedLinearComponent") { EltStage s; s.kind = EltStage::kRelu; st->push_back(s); return true; }
  if (c.type == "LogSoftmaxComponent") { EltStage s; s.kind = EltStage::kLogSoftmax; st->push_back(s); return true; }
  if (c.type == "BatchNormComponent") {
    // test-mode scale/offset exactly as BatchNormComponent::Read + ComputeDerived
    // (nnet-normalize-component.cc:209-246,590-612), float arithmetic
    int dim = c.Int("<Dim>"), block = c.Int("<BlockDim>");
    float eps = (float)c.f.at("<Epsilon>")[0], rms = (float)c.f.at("<TargetRms>")[0];
    double count = c.f.at("<Count>")[0];
    const std::vector<float> &mean = c.v.at("<StatsMean>"), &var = c.v.at("<StatsVar>");
    if (count == 0.0) Fail("nnet3: BatchNormComponent '" + name + "' has no stats (count = 0); cannot run in test mode");
    if ((int)mean.size() != block || (int)var.size() != block) Fail("nnet3: BatchNormComponent '" + name + "' stats dim mismatch");
    EltStage s;
    s.kind = EltStage::kScaleOffset;
    s.scale.resize(dim);
    s.offset.resize(dim);
    std::vector<float> sc(block), of(block);
    for (int i = 0; i < block; i++) {
      // Read(): stats_sumsq = (var + mean*mean) * count ; stats_sum = mean * count   [CuVector<float> ops]
      float sumsq = var[i] + mean[i] * mean[i];
      float ssum = mean[i] * (float)count;
      sumsq = sumsq * (float)count;
      // ComputeDerived()
      float off = ssum * (float)(-1.0 / count);
      float scl = sumsq * (float)(1.0 / count);
      scl = scl + (-1.0f) * off * off;
      if (scl < 0.0f) scl = 0.0f;
      scl = scl + eps;
      scl = powf(scl, -0.5f);
      scl = scl * rms;
      off = off * scl;
      sc[i] = scl;
      of[i] = off;
    }
    for (int i = 0; i < dim; i++) { s.scale[i] = sc[i % block]; s.offset[i] = of[i % block]; }
    st->push_back(s);
    return true;
  }
  if (c.type == "NormalizeComponent") {
    if (c.f.count("<AddLogStddev>") && c.f.at("<AddLogStddev>")[0] != 0.0) Fail("nnet3: NormalizeComponent add-log-stddev=true is not supported (node " + name + ")");
    if (c.f.count("<BlockDim>")) {
      int d = c.i.count("<InputDim>") ? c.Int("<InputDim>") : c.Int("<Dim>");
      if (c.Int("<BlockDim>") != d) Fail("nnet3: NormalizeComponent with block-dim is not supported (node " + name + ")");
    }
    EltStage s;
    s.kind = EltStage::kNormalize;
    s.alpha = c.f.count("<TargetRms>") ? (float)c.f.at("<TargetRms>")[0] : 1.0f;
    st->push_back(s);
    return true;
  }
  if (c.type == "FixedScaleComponent" || c.type == "PerElementScaleComponent" || c.type == "NaturalGradientPerElementScaleComponent") {
    const std::vector<float> &v = c.v.at(c.type == "FixedScaleComponent" ? "<Scales>" : "<Params>");
    EltStage s; s.kind = EltStage::kScaleOffset; s.scale = v; s.offset.assign(v.size(), 0.0f);
    st->push_back(s);
    return true;
  }
  if (c.type == "FixedBiasComponent" || c.type == "PerElementOffsetComponent") {
    const std::vector<float> &v = c.v.at(c.type == "FixedBiasComponent" ? "<Bias>" : "<Offsets>");
    if (c.type == "PerElementOffsetComponent" && c.f.count("<UseNaturalGradient>") == 0 && c.i.count("<Dim>") && c.Int("<Dim>") != (int)v.size())
      Fail("nnet3: PerElementOffsetComponent with block structure is not supported");
    EltStage s; s.kind = EltStage::kScaleOffset; s.offset = v; s.scale.assign(v.size(), 1.0f);
    st->push_back(s);
    return true;
  }
  if (c.type == "ScaleAndOffsetComponent") {
    std::vector<float> sc, of;
    ScaleAndOffsetVectors(c, name, &sc, &of);
    // the block form: <Dim> is a multiple of the vectors' length and they repeat along the row
    const int dim = c.Int("<Dim>"), block = (int)sc.size();
    EltStage s;
    s.kind = EltStage::kScaleOffset;
    s.scale.resize(dim);
    s.offset.resize(dim);
    for (int i = 0; i < dim; i++) { s.scale[i] = sc[i % block]; s.offset[i] = of[i % block]; }
    st->push_back(s);
    return true;
  }
  return false;
}

// The nodes of one recurrent block (xconfig/lstm.py: XconfigFastLstmpLayer :1120-1198, XconfigFastLstmLayer :706-753)
struct BlockNodes {
  int wa = -1, nl = -1, tr = -1, sc = -1, sr = -1;   // W_all, lstm_nonlin, cr_trunc / cm_trunc, c_trunc, r_trunc / m_trunc
  int c = -1, m = -1, rp = -1, r = -1;               // with a projection: the dim-ranges c and m, the affine rp, the dim-range r
  int dm = -1;                                       // the DropoutMaskComponent node (use-dropout=true); not part of the cycle
  int delay = 0, cell = 0, rec_dim = 0;              // rec_dim: width of the recurrent input (r, or m without a projection)
  int need_lext = 0;
  // a GRU block (xconfig/gru.py: XconfigFastOpgruLayer :1771-1866, XconfigFastNormOpgruLayer :1994-2111): wa = z_t_pre, nl = gru_nonlin_t,
  // sc = c_t (a dim-range of nl, read back unscaled), tr = sr = s_t; and
  bool gru = false;
  // a block around a GruNonlinearityComponent (XconfigFastPgruLayer, XconfigFastNormPgruLayer, XconfigFastGruLayer): the same fields with
  // the reset gate r in the output gate's place (wo = r_t_pre, os / od = its sigmoid / dropout node), no cdoto; without a projection
  // no wy, sp, nm either, and sc = y_t
  bool pgru = false;
  int wo = -1, zs = -1, os = -1, zd = -1, od = -1;   // o_t_pre, the two SigmoidComponent nodes, with dropout the two DropoutComponent nodes
  int hp = -1, cd = -1, wy = -1, sp = -1, nm = -1;   // hpart_t (not part of the cycle), cdoto, y_t / y_t_tmp, its dim-range, s_t_renorm (norm variant)
  // the composed LSTM(P) cell (xconfig/lstm.py: XconfigLstmpLayer, XconfigLstmLayer): tr = sc = c_t, sr = r_t, wa = i1_t (where the
  // block is placed); ga: the affine nodes i1_t, f1_t, g1_t, o1_t; pe: the peephole nodes i2_t, f2_t, o2_t; m = m_t; with a
  // projection rp = rp_t and r = r_t_preclip; cdrop: the shared DropoutComponent behind i, f and o is there
  bool composed = false, cdrop = false;
  int ga[4] = {-1, -1, -1, -1}, pe[3] = {-1, -1, -1};
  // the cell behind a bottleneck (xconfig/lstm.py: XconfigLstmbLayer): wa = W_all_a (where the block is placed), wb = W_all_b, so =
  // W_all_b_so, nl, tr = cm_trunc, sc / sr = c_trunc / m_trunc; self_scale: the Scale() on the recurrent input
  bool lstmb = false;
  int wb = -1, so = -1;
  float self_scale = 1.0f;
  // a GRU cell spelled out (xconfig/gru.py: XconfigGruLayer, XconfigPgruLayer, XconfigNormPgruLayer with pgru; XconfigOpgruLayer,
  // XconfigNormOpgruLayer with gru): the fields of the fast block, with sc = y_t (the NoOpComponent node, where the block is named),
  // nl = -1, and the cell's own nodes: ht = h_t, y1 / y2 = y1_t / y2_t; reset-gate family: hp = h_t_pre (part of the cycle, over
  // Append(x, h1_t)), h1 = h1_t; output-gate family: hp = h_t_pre (not part of the cycle), h2 = h_t_pre2, cd = y_o_t
  bool gruc = false;
  int ht = -1, y1 = -1, y2 = -1, h1 = -1, h2 = -1;
  std::vector<int> members;                         // the cycle's nodes (a GRU block: and hpart_t)
  std::vector<DescPart> x_parts;                     // W_all's input without its recurrent part
};

// Every cycle of the nodes `out_node` depends on has to be such a block, and nothing else: anything else is refused with the
// node and the reason.
void FindBlocks(const Nnet &net, int out_node, std::vector<BlockNodes> *blocks, std::vector<int> *block_of) {
  const std::vector<NnetNode> &nodes = net.nodes;
  const int N = (int)nodes.size();
  auto comp_type = [&](int n) -> std::string { return nodes[n].kind == NnetNode::kComponent ? net.components[nodes[n].component].type : std::string(); };
  auto deps = [&](int n, std::vector<int> *out) {
    out->clear();
    const NnetNode &nd = nodes[n];
    if (comp_type(n) == "DropoutMaskComponent") return;      // (its input is a don't-care: GetInputIndexes asks for nothing)
    if (nd.kind == NnetNode::kDimRange) out->push_back(nd.range_node);
    for (auto &p : nd.input.parts) for (auto &t : p.terms) if (!t.konst) out->push_back(t.node);
  };
  // strongly connected components (Tarjan, iterative over an explicit stack) of what the output depends on
  std::vector<int> index(N, -1), low(N, 0), comp(N, -1), stack;
  std::vector<char> on_stack(N, 0);
  int counter = 0, ncomp = 0;
  std::vector<std::vector<int>> sccs;
  struct Frame { int n; std::vector<int> d; size_t i; };
  std::vector<Frame> call;
  auto push = [&](int n) {
    index[n] = low[n] = counter++;
    stack.push_back(n);
    on_stack[n] = 1;
    Frame f{n, {}, 0};
    deps(n, &f.d);
    call.push_back(std::move(f));
  };
  push(out_node);
  while (!call.empty()) {
    Frame &f = call.back();
    if (f.i < f.d.size()) {
      const int m = f.d[f.i++];
      if (index[m] < 0) push(m);
      else if (on_stack[m]) low[f.n] = std::min(low[f.n], index[m]);
      continue;
    }
    const int n = f.n;
    if (low[n] == index[n]) {
      std::vector<int> scc;
      for (;;) {
        const int m = stack.back();
        stack.pop_back();
        on_stack[m] = 0;
        comp[m] = ncomp;
        scc.push_back(m);
        if (m == n) break;
      }
      ncomp++;
      std::sort(scc.begin(), scc.end());
      sccs.push_back(std::move(scc));
    }
    call.pop_back();
    if (!call.empty()) low[call.back().n] = std::min(low[call.back().n], low[n]);
  }
  block_of->assign(N, -1);
  for (const std::vector<int> &scc : sccs) {
    if (scc.size() == 1) {
      std::vector<int> d;
      deps(scc[0], &d);
      if (std::find(d.begin(), d.end(), scc[0]) == d.end()) continue;
    }
    auto in_scc = [&](int n) { return std::binary_search(scc.begin(), scc.end(), n); };
    // (a cycle that holds one of the two GRU nonlinearities is the GRU recogniser's, with wording of its own)
    bool gru_cycle = false;
    for (int n : scc) gru_cycle = gru_cycle || comp_type(n) == "OutputGruNonlinearityComponent" || comp_type(n) == "GruNonlinearityComponent";
    // (... and one that holds a GruNonlinearityComponent has to be a fast-pgru / fast-norm-pgru / fast-gru block)
    bool pgru_cycle = false;
    for (int n : scc) pgru_cycle = pgru_cycle || comp_type(n) == "GruNonlinearityComponent";
    // (... and one that holds none of the three nonlinearities but a NoOpComponent node is a GRU cell spelled out: only gru-layer,
    // pgru-layer, opgru-layer and their norm forms have that node, y_t; lstm.py emits none)
    bool gruc_cycle = !gru_cycle;
    for (int n : scc) gruc_cycle = gruc_cycle && comp_type(n) != "LstmNonlinearityComponent";
    if (gruc_cycle) {
      gruc_cycle = false;
      for (int n : scc) gruc_cycle = gruc_cycle || comp_type(n) == "NoOpComponent";
    }
    auto refuse = [&](int n, const std::string &why) {
      if (gruc_cycle)
        Fail("nnet3: a recurrent cycle without a nonlinearity component but with a NoOpComponent node is supported only as one gru-layer / pgru-layer / "
             "norm-pgru-layer / opgru-layer / norm-opgru-layer block (cycle at node " + nodes[n].name + ": " + why + ")");
      if (pgru_cycle)
        Fail("nnet3: recurrent GRU networks are supported only as fast-opgru-layer / fast-norm-opgru-layer blocks and, around a GruNonlinearityComponent, as "
             "fast-pgru-layer / fast-norm-pgru-layer / fast-gru-layer blocks (cycle at node " + nodes[n].name + ": " + why + ")");
      if (gru_cycle)
        Fail("nnet3: recurrent GRU networks are supported only as fast-opgru-layer / fast-norm-opgru-layer blocks (cycle at node " + nodes[n].name + ": " + why + ")");
      Fail("nnet3: recurrent networks are supported only as fast-lstmp-layer / fast-lstm-layer blocks (cycle at node " + nodes[n].name + ": " + why + ")");
    };
    BlockNodes b;
    for (int n : scc)
      if (comp_type(n) == "LstmNonlinearityComponent") {
        if (b.nl >= 0) refuse(n, "a second LstmNonlinearityComponent in one cycle");
        b.nl = n;
      }
    // (a cycle without any of the three nonlinearities has to be the same cell spelled out: lstmp-layer / lstm-layer, below)
    const bool composed_cycle = b.nl < 0 && !gru_cycle && !gruc_cycle;
    // a recurrent part: one optional term, Offset(x, -d) with 1 <= d <= kLstmMaxDelay
    // (self_scale: where given, the term may be Offset(Scale(s, node), -d) and s is returned there -- an lstmb-layer block only)
    auto recurrent_part = [&](int at, const DescPart &p, int *node, float *self_scale = nullptr) {
      if (p.terms.size() != 1 || p.terms[0].const_t || p.terms[0].konst || (p.terms[0].scale != 1.0f && !self_scale)) refuse(at, "its recurrent input is not IfDefined(Offset(node, -delay))");
      if (self_scale) *self_scale = p.terms[0].scale;
      const DescTerm &t = p.terms[0];
      if (!t.optional) refuse(at, "its recurrent input " + nodes[t.node].name + " is not inside IfDefined()");
      if (t.offset > 0) refuse(at, "a positive delay, Offset(" + nodes[t.node].name + ", " + std::to_string(t.offset) + "): a recurrence towards the future is not supported");
      if (t.offset == 0 || -t.offset > kLstmMaxDelay)
        refuse(at, "a delay of " + std::to_string(-t.offset) + " frames; the HIP kernel takes 1 to " + std::to_string(kLstmMaxDelay));
      *node = t.node;
      return -t.offset;
    };
    auto plain_part = [&](const DescPart &p) { return p.terms.size() == 1 && !p.terms[0].const_t && !p.terms[0].konst && !p.terms[0].optional && p.terms[0].offset == 0 && p.terms[0].scale == 1.0f; };
    auto range_of = [&](int n, int src, int off, int dim) { return nodes[n].kind == NnetNode::kDimRange && nodes[n].range_node == src && nodes[n].range_offset == off && nodes[n].dim == dim; };
    auto only_input = [&](int n) { const NnetNode &nd = nodes[n]; return nd.input.parts.size() == 1 && plain_part(nd.input.parts[0]) ? nd.input.parts[0].terms[0].node : -1; };
    auto is_affine = [&](int n) { const std::string t = comp_type(n); return t == "AffineComponent" || t == "NaturalGradientAffineComponent"; };
    auto same_parts = [&](const std::vector<DescPart> &a, size_t na, const std::vector<DescPart> &c) {
      if (na != c.size()) return false;
      for (size_t i = 0; i < na; i++) {
        if (a[i].dim != c[i].dim || a[i].terms.size() != c[i].terms.size()) return false;
        for (size_t j = 0; j < a[i].terms.size(); j++) {
          const DescTerm &s = a[i].terms[j], &t = c[i].terms[j];
          if (s.node != t.node || s.offset != t.offset || s.scale != t.scale || s.const_t != t.const_t || s.konst != t.konst || s.optional != t.optional) return false;
        }
      }
      return true;
    };
    if (gruc_cycle) {
      // ---- a GRU cell spelled out (xconfig/gru.py: XconfigGruLayer :36-169, XconfigPgruLayer :197-371, XconfigNormPgruLayer :400-605,
      // XconfigOpgruLayer :631-806, XconfigNormOpgruLayer :834-1045), found from its NoOpComponent node y_t
      auto is_trunc = [&](int n) { const std::string t = comp_type(n); return t == "BackpropTruncationComponent" || t == "ClipGradientComponent"; };
      auto is_product = [&](int n, int dim) { return n >= 0 && comp_type(n) == "ElementwiseProductComponent" && nodes[n].dim == dim && nodes[n].input.dim == 2 * dim; };
      int y_t = -1;
      for (int n : scc)
        if (comp_type(n) == "NoOpComponent") {
          if (y_t >= 0) refuse(n, "a second NoOpComponent node in one cycle");
          y_t = n;
        }
      b.gruc = true;
      b.sc = y_t;
      const int C = b.cell = nodes[y_t].dim;
      // y_t = NoOp(Sum(y1_t, y2_t))
      {
        const NnetNode &yn = nodes[y_t];
        bool ok = yn.input.parts.size() == 1 && yn.input.parts[0].terms.size() == 2;
        if (ok) for (auto &t : yn.input.parts[0].terms) ok = ok && !t.const_t && !t.konst && !t.optional && t.offset == 0 && t.scale == 1.0f;
        if (!ok) refuse(y_t, "its input is not Sum(y1_t, y2_t)");
        b.y1 = yn.input.parts[0].terms[0].node;
        b.y2 = yn.input.parts[0].terms[1].node;
      }
      if (!is_product(b.y1, C) || !is_product(b.y2, C)) refuse(y_t, "its input is not the Sum() of two ElementwiseProductComponent nodes of the cell's dim");
      // y1_t = Append(h_t, Sum(Scale(-1.0, z_t), Const(1.0, cell)))
      const NnetNode &y1n = nodes[b.y1];
      if (y1n.input.parts.size() != 2 || !plain_part(y1n.input.parts[0]) || y1n.input.parts[1].terms.size() != 2)
        refuse(b.y1, "its input is not Append(h_t, Sum(Scale(-1.0, z_t), Const(1.0, cell-dim)))");
      b.ht = y1n.input.parts[0].terms[0].node;
      const DescTerm &zt = y1n.input.parts[1].terms[0], &one = y1n.input.parts[1].terms[1];
      if (zt.konst || zt.const_t || zt.optional || zt.offset != 0 || !one.konst)
        refuse(b.y1, "its second input is not Sum(Scale(-1.0, z_t), Const(1.0, cell-dim)), in that order");
      if (zt.scale != -1.0f) refuse(b.y1, "its second input scales " + nodes[zt.node].name + " by " + std::to_string(zt.scale) + ", not by -1.0: it is not 1 - z_t");
      if (one.scale != 1.0f) refuse(b.y1, "its second input adds Const(" + std::to_string(one.scale) + "), not Const(1.0): it is not 1 - z_t");
      const int z_t = zt.node;
      // y2_t = Append(IfDefined(Offset(y_t, -d)), z_t); gru-layer reads s_t there
      const NnetNode &y2n = nodes[b.y2];
      if (y2n.input.parts.size() != 2) refuse(b.y2, "its input is not Append(IfDefined(Offset(y_t, -delay)), z_t)");
      int y_prev = -1;
      b.delay = recurrent_part(b.y2, y2n.input.parts[0], &y_prev);
      if (!plain_part(y2n.input.parts[1]) || y2n.input.parts[1].terms[0].node != z_t)
        refuse(b.y2, "its second input is not the update gate " + nodes[z_t].name + " that y1_t reads");
      auto state_part = [&](int at, const DescPart &p, int want, const char *role) {
        int node = -1;
        const int d2 = recurrent_part(at, p, &node);
        if (d2 != b.delay) refuse(at, "two different delays in one block, " + std::to_string(d2) + " and " + std::to_string(b.delay));
        if (want >= 0 && node != want) refuse(at, std::string(role) + " reads " + nodes[node].name + ", not " + nodes[want].name);
        return node;
      };
      // a gate: [DropoutComponent over] a SigmoidComponent over an affine over Append(x, IfDefined(Offset(s_t, -d)))
      auto gate = [&](int g, int rows, const char *rows_name, int *drop, int *sig, int *aff) {
        *drop = -1;
        if (comp_type(g) == "DropoutComponent") {
          *drop = g;
          g = only_input(g);
          if (g < 0) refuse(*drop, "the dropout's input is not one node");
        }
        if (comp_type(g) != "SigmoidComponent") refuse(g, "the gate is not a SigmoidComponent node [behind a DropoutComponent]");
        *sig = g;
        const int a = only_input(g);
        if (a < 0 || !is_affine(a)) refuse(g, "the sigmoid's input is not an affine component node");
        *aff = a;
        const NnetNode &an = nodes[a];
        if (an.input.parts.size() < 2) refuse(a, "its input is not Append(x, IfDefined(Offset(s_t, -delay)))");
        const int state = state_part(a, an.input.parts.back(), b.tr, "the gate");
        if (b.tr < 0) b.tr = b.sr = state;
        if (rows > 0 && an.dim != rows) refuse(a, "the gate's affine has " + std::to_string(an.dim) + " rows, not the " + rows_name + " " + std::to_string(rows));
      };
      gate(z_t, C, "cell's dim", &b.zd, &b.zs, &b.wa);
      if (!is_trunc(b.tr)) refuse(b.tr, "the recurrent state does not come through a BackpropTruncationComponent / ClipGradientComponent");
      const int R = b.rec_dim = nodes[b.tr].dim;
      const NnetNode &wz = nodes[b.wa];
      b.x_parts.assign(wz.input.parts.begin(), wz.input.parts.end() - 1);
      // h_t: a TanhComponent over the affine h_t_pre (the reset-gate family) or over Sum(h_t_pre, h_t_pre2) (the output-gate family)
      if (comp_type(b.ht) != "TanhComponent") refuse(b.ht, "h_t is not a TanhComponent node");
      const NnetNode &htn = nodes[b.ht];
      const bool out_gate = htn.input.parts.size() == 1 && htn.input.parts[0].terms.size() == 2;
      int src = only_input(b.tr);
      bool proj = true;
      if (!out_gate) {
        b.pgru = true;
        b.hp = only_input(b.ht);
        if (b.hp < 0 || !is_affine(b.hp)) refuse(b.ht, "h_t's input is neither an affine component node nor the Sum() of one and a per-element scale");
        const NnetNode &hp = nodes[b.hp];
        if (hp.input.parts.size() < 2 || !plain_part(hp.input.parts.back())) refuse(b.hp, "its input is not Append(x, h1_t)");
        b.h1 = hp.input.parts.back().terms[0].node;
        if (!is_product(b.h1, R)) refuse(b.h1, "h1_t is not an ElementwiseProductComponent node of the recurrent state's dim " + std::to_string(R));
        const NnetNode &h1n = nodes[b.h1];
        if (h1n.input.parts.size() != 2 || !plain_part(h1n.input.parts[0])) refuse(b.h1, "its input is not Append(r_t, IfDefined(Offset(s_t, -delay)))");
        state_part(b.h1, h1n.input.parts[1], b.tr, "the product h1_t");
        gate(h1n.input.parts[0].terms[0].node, R, "recurrent dim", &b.od, &b.os, &b.wo);
        if (!same_parts(hp.input.parts, hp.input.parts.size() - 1, b.x_parts)) refuse(b.hp, "h_t_pre does not read the gates' feed-forward input");
        if (hp.dim != C) refuse(b.hp, "h_t_pre has " + std::to_string(hp.dim) + " rows, not the cell's dim " + std::to_string(C));
        if (src == y_t) {      // gru-layer: s_t = s_r(y_t), and y2_t reads s_t
          proj = false;
          if (R != C) refuse(b.tr, "without a projection the recurrent state is of the cell's dim");
          if (y_prev != b.tr) refuse(b.y2, "the product y2_t reads " + nodes[y_prev].name + ", not " + nodes[b.tr].name + " as in gru-layer");
        }
      } else {
        b.gru = true;
        for (auto &t : htn.input.parts[0].terms) if (t.const_t || t.konst || t.optional || t.offset != 0 || t.scale != 1.0f) refuse(b.ht, "h_t's input is not Sum(h_t_pre, h_t_pre2)");
        b.hp = htn.input.parts[0].terms[0].node;
        b.h2 = htn.input.parts[0].terms[1].node;
        const std::string pt = comp_type(b.h2);
        if (!is_affine(b.hp) || (pt != "NaturalGradientPerElementScaleComponent" && pt != "PerElementScaleComponent"))
          refuse(b.ht, "h_t's input is not Sum(affine node, per-element scale node)");
        const NnetNode &hp = nodes[b.hp], &h2n = nodes[b.h2];
        if (!same_parts(hp.input.parts, hp.input.parts.size(), b.x_parts)) refuse(b.hp, "h_t_pre is not an affine component node over the gates' feed-forward input");
        if (hp.dim != C) refuse(b.hp, "h_t_pre has " + std::to_string(hp.dim) + " rows, not the cell's dim " + std::to_string(C));
        if (h2n.dim != C || h2n.input.parts.size() != 1) refuse(b.h2, "h_t_pre2 is not of the cell's dim over one input");
        state_part(b.h2, h2n.input.parts[0], y_t, "the per-element scale h_t_pre2");
      }
      if (proj) {
        if (y_prev != y_t) refuse(b.y2, "the product y2_t reads " + nodes[y_prev].name + ", not " + nodes[y_t].name);
        if (src >= 0 && comp_type(src) == "NormalizeComponent") {
          b.nm = src;
          const Component &nmc = net.components[nodes[b.nm].component];
          if (nmc.f.count("<AddLogStddev>") && nmc.f.at("<AddLogStddev>")[0] != 0.0) refuse(b.nm, "a NormalizeComponent with add-log-stddev=true is not supported");
          if (nmc.f.count("<BlockDim>") && nmc.Int("<BlockDim>") != (nmc.i.count("<InputDim>") ? nmc.Int("<InputDim>") : nmc.Int("<Dim>")))
            refuse(b.nm, "a NormalizeComponent with block-dim is not supported");
          src = only_input(b.nm);
        }
        if (src < 0 || nodes[src].kind != NnetNode::kDimRange) refuse(b.tr, "the recurrent state is neither y_t nor a dim-range of W_s.ys' node [through a NormalizeComponent]");
        b.sp = src;
        b.wy = nodes[b.sp].range_node;
        if (!is_affine(b.wy) || !range_of(b.sp, b.wy, 0, R)) refuse(b.sp, "the recurrent state is not the first recurrent-dim columns of an affine component node");
        int y_in = only_input(b.wy);
        if (out_gate) {
          b.cd = y_in;
          int o_t = -1;
          if (!is_product(b.cd, C)) refuse(b.wy, "W_s.ys' input is not the ElementwiseProductComponent node y_o_t of the cell's dim");
          const NnetNode &cd = nodes[b.cd];
          if (cd.input.parts.size() != 2 || !plain_part(cd.input.parts[0]) || !plain_part(cd.input.parts[1]) || cd.input.parts[1].terms[0].node != y_t)
            refuse(b.cd, "the product's input is not Append(o_t, y_t)");
          o_t = cd.input.parts[0].terms[0].node;
          gate(o_t, C, "cell's dim", &b.od, &b.os, &b.wo);
        } else if (y_in != y_t) {
          refuse(b.wy, "W_s.ys' input is not the cell " + nodes[y_t].name);
        }
      }
      if ((b.zd >= 0) != (b.od >= 0)) refuse(b.zd >= 0 ? b.zd : b.od, "only one of the two gates has a DropoutComponent");
      if (!same_parts(nodes[b.wo].input.parts, nodes[b.wo].input.parts.size() - 1, b.x_parts)) refuse(b.wo, "the two gates do not read the same feed-forward input");
      for (auto &p : b.x_parts) for (auto &t : p.terms) if (t.konst || in_scc(t.node)) refuse(b.wa, "its feed-forward input reads a Const() or a node of the cycle");
      b.members = {b.wa, b.wo, b.zs, b.os, b.ht, b.y1, b.y2, y_t, b.tr};
      for (int n : {b.zd, b.od, b.nm, b.wy, b.sp, b.cd, b.h1, b.h2}) if (n >= 0) b.members.push_back(n);
      if (b.pgru) b.members.push_back(b.hp);
      std::sort(b.members.begin(), b.members.end());
      if (std::adjacent_find(b.members.begin(), b.members.end()) != b.members.end()) refuse(y_t, "a node has two roles in the block");
      for (int n : scc) if (!std::binary_search(b.members.begin(), b.members.end(), n)) refuse(n, "the node is part of the cycle but not of such a block");
      for (int n : b.members) if (!in_scc(n)) refuse(n, "the node is not part of the cycle");
      if (b.gru && (in_scc(b.hp) || (*block_of)[b.hp] >= 0)) refuse(b.hp, "h_t_pre is part of a cycle");
      // dims against the weights
      int x_dim = 0;
      for (auto &p : b.x_parts) x_dim += p.dim;
      for (int a : {b.wa, b.wo, b.hp}) {
        const MatF &W = net.components[nodes[a].component].m.at("<LinearParams>");
        const int rec_cols = a == b.hp && b.gru ? 0 : R;
        if (W.rows != nodes[a].dim || W.cols != x_dim + rec_cols)
          refuse(a, "its weights are " + std::to_string(W.rows) + " x " + std::to_string(W.cols) + ", the block needs " + std::to_string(nodes[a].dim) + " rows and the feed-forward input's " +
                        std::to_string(x_dim) + " + the recurrent input's " + std::to_string(rec_cols) + " columns");
      }
      if (b.gru) {
        const Component &pc = net.components[nodes[b.h2].component];
        auto pit = pc.v.find("<Params>");
        if (pit == pc.v.end() || (int)pit->second.size() != C) refuse(b.h2, "the per-element scale's <Params> are not a vector of the cell's dim " + std::to_string(C));
      }
      if (b.wy >= 0) {
        const MatF &Wy = net.components[nodes[b.wy].component].m.at("<LinearParams>");
        if (Wy.cols != C || Wy.rows < R || Wy.rows != nodes[b.wy].dim) refuse(b.wy, "W_s.ys is " + std::to_string(Wy.rows) + " x " + std::to_string(Wy.cols) + ", the block needs cell-dim columns and at least the recurrent dim's rows");
      }
      // only what has a buffer may be read from outside the block: y_t, W_s.ys' node, its dim-range and the state
      for (int n = 0; n < N; n++) {
        if (std::binary_search(b.members.begin(), b.members.end(), n) || index[n] < 0 || n == b.hp) continue;
        std::vector<int> d;
        deps(n, &d);
        for (int m : d)
          if ((m == b.hp || std::binary_search(b.members.begin(), b.members.end(), m)) && m != y_t && m != b.wy && m != b.sp && m != b.tr)
            refuse(m, "the node is read from outside the block, by " + nodes[n].name);
      }
      if (b.gru) { b.members.push_back(b.hp); std::sort(b.members.begin(), b.members.end()); }
      for (int n : b.members) (*block_of)[n] = (int)blocks->size();
      blocks->push_back(std::move(b));
      continue;
    }
    if (composed_cycle) {
      // ---- the composed LSTM(P) cell (xconfig/lstm.py: XconfigLstmpLayer :440-565, XconfigLstmLayer :160-255)
      auto no = [&](int n, const std::string &why) {
        refuse(n, "the cycle has no LstmNonlinearityComponent and is no complete lstmp-layer / lstm-layer block (four affines, three peepholes, Sigmoid / Tanh / "
                  "ElementwiseProduct components, two truncation components) either; the non-fast GRU layers are not supported: " + why);
      };
      auto is_trunc = [&](int n) { const std::string t = comp_type(n); return t == "BackpropTruncationComponent" || t == "ClipGradientComponent"; };
      auto is_peephole = [&](int n) { const std::string t = comp_type(n); return t == "NaturalGradientPerElementScaleComponent" || t == "PerElementScaleComponent"; };
      auto two_plain = [&](int n, int *x, int *y) {      // Append(x, y) of two plain nodes
        const NnetNode &nd = nodes[n];
        if (nd.input.parts.size() != 2 || !plain_part(nd.input.parts[0]) || !plain_part(nd.input.parts[1])) return false;
        *x = nd.input.parts[0].terms[0].node;
        *y = nd.input.parts[1].terms[0].node;
        return true;
      };
      auto two_sum = [&](int n, int *x, int *y) {        // Sum(x, y) of two plain nodes
        const NnetNode &nd = nodes[n];
        if (nd.input.parts.size() != 1 || nd.input.parts[0].terms.size() != 2) return false;
        for (auto &t : nd.input.parts[0].terms) if (t.const_t || t.konst || t.optional || t.offset != 0 || t.scale != 1.0f) return false;
        *x = nd.input.parts[0].terms[0].node;
        *y = nd.input.parts[0].terms[1].node;
        return true;
      };
      b.composed = true;
      // the two truncation nodes: c_t over Sum(c1_t, c2_t), r_t over one node
      int c_t = -1, r_t = -1, c1 = -1, c2 = -1;
      for (int n : scc) {
        if (!is_trunc(n)) continue;
        int x, y;
        if (two_sum(n, &x, &y)) {
          if (c_t >= 0) no(n, "a second truncation node over a Sum() in one cycle");
          c_t = n; c1 = x; c2 = y;
        } else {
          if (r_t >= 0) no(n, "a second truncation node over one node in one cycle");
          r_t = n;
        }
      }
      if (c_t < 0) no(scc[0], "it has no cell node c_t, a BackpropTruncationComponent / ClipGradientComponent over Sum(c1_t, c2_t)");
      if (r_t < 0) no(c_t, "it has no recurrent state node r_t, a BackpropTruncationComponent / ClipGradientComponent over r_t_preclip or m_t");
      const int C = b.cell = nodes[c_t].dim;
      b.tr = b.sc = c_t;
      b.sr = r_t;
      b.delay = 0;
      // a recurrent input of the block: IfDefined(Offset(want, -d)), one d
      auto state_part = [&](int at, const DescPart &p, int want, const char *role) {
        int node = -1;
        const int d2 = recurrent_part(at, p, &node);
        if (b.delay == 0) b.delay = d2;
        if (d2 != b.delay) refuse(at, "two different delays in one block, " + std::to_string(d2) + " and " + std::to_string(b.delay));
        if (node != want) no(at, std::string(role) + " reads " + nodes[node].name + ", not " + nodes[want].name);
      };
      auto is_product = [&](int n) { return comp_type(n) == "ElementwiseProductComponent" && nodes[n].dim == C && nodes[n].input.dim == 2 * C; };
      // c1_t = Append(f_t, IfDefined(Offset(c_t, -d))), c2_t = Append(i_t, g_t)
      if (!is_product(c1) || !is_product(c2)) no(c_t, "its input is not the Sum() of two ElementwiseProductComponent nodes of the cell's dim");
      const NnetNode &c1n = nodes[c1];
      if (c1n.input.parts.size() != 2 || !plain_part(c1n.input.parts[0])) no(c1, "its input is not Append(f_t, IfDefined(Offset(c_t, -delay)))");
      const int f_t = c1n.input.parts[0].terms[0].node;
      state_part(c1, c1n.input.parts[1], c_t, "the product c1_t");
      int i_t = -1, g_t = -1;
      if (!two_plain(c2, &i_t, &g_t)) no(c2, "its input is not Append(i_t, g_t)");
      // the recurrent state: r_t over the dim-range of W_rp.m's node, or over m_t
      int m_t = only_input(r_t);
      if (m_t < 0) no(r_t, "its input is not one node");
      if (nodes[m_t].kind == NnetNode::kDimRange) {
        b.r = m_t;
        b.rp = nodes[b.r].range_node;
        b.rec_dim = nodes[b.r].dim;
        if (!is_affine(b.rp) || !range_of(b.r, b.rp, 0, b.rec_dim) || nodes[r_t].dim != b.rec_dim) no(b.r, "the recurrent state is not the first columns of an affine component node");
        m_t = only_input(b.rp);
        if (m_t < 0) no(b.rp, "the projection's input is not m_t");
      } else {
        b.rec_dim = C;
        if (nodes[r_t].dim != C) no(r_t, "without a projection the recurrent state is m_t, of the cell's dim");
      }
      b.m = m_t;
      int o_t = -1, h_t = -1;
      if (!is_product(m_t) || !two_plain(m_t, &o_t, &h_t)) no(m_t, "m_t is not an ElementwiseProductComponent node over Append(o_t, h_t)");
      if (comp_type(h_t) != "TanhComponent" || only_input(h_t) != c_t) no(h_t, "h_t is not a TanhComponent node over the cell " + nodes[c_t].name);
      if (comp_type(g_t) != "TanhComponent") no(g_t, "g_t is not a TanhComponent node");
      b.ga[2] = only_input(g_t);
      if (b.ga[2] < 0 || !is_affine(b.ga[2])) no(g_t, "g_t's input is not an affine component node");
      // a gate: [the shared DropoutComponent over] a SigmoidComponent over Sum(affine node, peephole node)
      int drop[3] = {-1, -1, -1}, sig[3] = {-1, -1, -1};
      auto gate = [&](int g, int which, const char *gname) {
        if (comp_type(g) == "DropoutComponent") {
          drop[which] = g;
          g = only_input(g);
          if (g < 0) no(drop[which], "the dropout's input is not one node");
        }
        if (comp_type(g) != "SigmoidComponent") no(g, std::string(gname) + " is not a SigmoidComponent node [behind a DropoutComponent]");
        sig[which] = g;
        int a = -1, pe = -1;
        if (!two_sum(g, &a, &pe) || !is_affine(a) || !is_peephole(pe)) no(g, "its input is not Sum(affine node, peephole node)");
        b.ga[which == 2 ? 3 : which] = a;
        b.pe[which] = pe;
        const NnetNode &pn = nodes[pe];
        if (pn.dim != C || pn.input.parts.size() != 1) no(pe, "the peephole is not of the cell's dim over one input");
        if (which == 2) {      // w_o.c reads the current, already scaled cell
          if (only_input(pe) != c_t) no(pe, "the output gate's peephole does not read the current cell " + nodes[c_t].name);
        } else {
          if (plain_part(pn.input.parts[0])) no(pe, "the peephole reads " + nodes[pn.input.parts[0].terms[0].node].name + " of the current row, not IfDefined(Offset(" + nodes[c_t].name + ", -delay))");
          state_part(pe, pn.input.parts[0], c_t, "the peephole");
        }
      };
      gate(i_t, 0, "i_t");
      gate(f_t, 1, "f_t");
      gate(o_t, 2, "o_t");
      if ((drop[0] >= 0) != (drop[1] >= 0) || (drop[0] >= 0) != (drop[2] >= 0) ||
          (drop[0] >= 0 && (nodes[drop[0]].component != nodes[drop[1]].component || nodes[drop[0]].component != nodes[drop[2]].component)))
        no(drop[0] >= 0 ? drop[0] : drop[1] >= 0 ? drop[1] : drop[2], "the three gates do not share one DropoutComponent");
      b.cdrop = drop[0] >= 0;
      // the four affines: Append(x, IfDefined(Offset(r_t, -d))) over one feed-forward input
      for (int a = 0; a < 4; a++) {
        const NnetNode &an = nodes[b.ga[a]];
        if (an.input.parts.size() < 2) no(b.ga[a], "its input is not Append(x, IfDefined(Offset(r_t, -delay)))");
        state_part(b.ga[a], an.input.parts.back(), r_t, "the affine");
        if (an.dim != C) no(b.ga[a], "the affine has " + std::to_string(an.dim) + " rows, not the cell's dim " + std::to_string(C));
        if (a == 0) b.x_parts.assign(an.input.parts.begin(), an.input.parts.end() - 1);
        else if (!same_parts(an.input.parts, an.input.parts.size() - 1, b.x_parts)) no(b.ga[a], "the four gates do not read the same feed-forward input");
      }
      b.wa = b.ga[0];
      for (auto &p : b.x_parts) for (auto &t : p.terms) if (in_scc(t.node)) no(b.wa, "its feed-forward input reads " + nodes[t.node].name + ", a node of the cycle");
      b.members = {c_t, r_t, c1, c2, m_t, h_t, g_t, b.ga[0], b.ga[1], b.ga[2], b.ga[3], b.pe[0], b.pe[1], b.pe[2], sig[0], sig[1], sig[2]};
      for (int n : {drop[0], drop[1], drop[2], b.rp, b.r}) if (n >= 0) b.members.push_back(n);
      std::sort(b.members.begin(), b.members.end());
      if (std::adjacent_find(b.members.begin(), b.members.end()) != b.members.end()) no(c_t, "a node has two roles in the block");
      for (int n : scc) if (!std::binary_search(b.members.begin(), b.members.end(), n)) no(n, "the node is part of the cycle but not of such a block");
      for (int n : b.members) if (!in_scc(n)) no(n, "the node is not part of the cycle");
      // dims against the weights
      int x_dim = 0;
      for (auto &p : b.x_parts) x_dim += p.dim;
      for (int a = 0; a < 4; a++) {
        const MatF &W = net.components[nodes[b.ga[a]].component].m.at("<LinearParams>");
        if (W.rows != C || W.cols != x_dim + b.rec_dim)
          no(b.ga[a], "its weights are " + std::to_string(W.rows) + " x " + std::to_string(W.cols) + ", the block needs cell-dim rows and the feed-forward input's " +
                          std::to_string(x_dim) + " + the recurrent input's " + std::to_string(b.rec_dim) + " columns");
      }
      for (int g = 0; g < 3; g++) {
        const Component &pc = net.components[nodes[b.pe[g]].component];
        auto pit = pc.v.find("<Params>");
        if (pit == pc.v.end() || (int)pit->second.size() != C) no(b.pe[g], "the peephole's <Params> are not a vector of the cell's dim " + std::to_string(C));
      }
      if (b.rp >= 0) {
        const MatF &Wrp = net.components[nodes[b.rp].component].m.at("<LinearParams>");
        if (Wrp.cols != C || Wrp.rows < b.rec_dim) no(b.rp, "W_rp is " + std::to_string(Wrp.rows) + " x " + std::to_string(Wrp.cols) + ", the block needs cell-dim columns and at least the recurrent dim's rows");
      }
      // only the output has a buffer the layers above may read: rp_t, or m_t (without a projection; with one, where the collapser
      // has folded a W_rp.m that does not reduce the dim into the affine above, which then reads m_t)
      for (int n = 0; n < N; n++) {
        if (std::binary_search(b.members.begin(), b.members.end(), n) || index[n] < 0) continue;
        std::vector<int> d;
        deps(n, &d);
        for (int m : d)
          if (m != b.rp && m != m_t && std::binary_search(b.members.begin(), b.members.end(), m)) no(m, "the node is read from outside the block, by " + nodes[n].name);
      }
      for (int n : b.members) (*block_of)[n] = (int)blocks->size();
      blocks->push_back(std::move(b));
      continue;
    }
    if (pgru_cycle) {
      // ---- a block around a GruNonlinearityComponent (xconfig/gru.py: XconfigFastGruLayer, XconfigFastPgruLayer, XconfigFastNormPgruLayer)
      const std::string kWhat = "a GruNonlinearityComponent (fast-gru-layer, fast-pgru-layer, fast-norm-pgru-layer) ";
      b.pgru = true;
      b.nl = -1;
      for (int n : scc)
        if (comp_type(n) == "GruNonlinearityComponent") {
          if (b.nl >= 0) refuse(n, "a second GruNonlinearityComponent in one cycle");
          b.nl = n;
        }
      // the nonlinearity: Append(z_t, r_t, hpart_t, IfDefined(Offset(c_t, -d)), IfDefined(Offset(s_t, -d))); without a projection
      // Append(z_t, r_t, hpart_t, IfDefined(Offset(s_t, -d)))
      const NnetNode &nl = nodes[b.nl];
      const Component &nc = net.components[nl.component];
      const int C = b.cell = nl.dim / 2;
      const size_t n_parts = nl.input.parts.size();
      if (!nc.i.count("<RecurrentDim>") || nc.Int("<RecurrentDim>") <= 0)
        refuse(b.nl, kWhat + "without a <RecurrentDim>, over an input of " + std::to_string(n_parts) + " parts");
      const int R = b.rec_dim = nc.Int("<RecurrentDim>");
      const bool proj = n_parts == 5;
      if (n_parts != 4 && n_parts != 5)
        refuse(b.nl, kWhat + "whose input has " + std::to_string(n_parts) + " parts, not Append(z_t, r_t, hpart_t, [IfDefined(Offset(c_t, -delay)),] IfDefined(Offset(s_t, -delay)))");
      if (!proj && R != C)
        refuse(b.nl, kWhat + "with <RecurrentDim> " + std::to_string(R) + " and <CellDim> " + std::to_string(C) + " over a four-part input: without a projection the two are equal");
      {
        // <w_h>: cell x R (a one-row text matrix lands in the vector map)
        auto mit = nc.m.find("<w_h>");
        auto vit = nc.v.find("<w_h>");
        const int rows = mit != nc.m.end() ? mit->second.rows : vit != nc.v.end() && !vit->second.empty() ? 1 : 0;
        const int cols = mit != nc.m.end() ? mit->second.cols : vit != nc.v.end() ? (int)vit->second.size() : 0;
        if (rows != C || cols != R)
          refuse(b.nl, kWhat + "whose <w_h> is " + std::to_string(rows) + " x " + std::to_string(cols) + ", not cell-dim " + std::to_string(C) + " x recurrent-dim " + std::to_string(R));
      }
      const int part_dims[5] = {C, R, C, C, R};      // (without a projection R = C: the fourth part is s_t)
      for (size_t i = 0; i < n_parts; i++)
        if (nl.input.parts[i].dim != part_dims[i]) refuse(b.nl, kWhat + "whose input parts are not of the dims cell, recurrent, cell, [cell,] recurrent");
      for (int i = 0; i < 3; i++)
        if (!plain_part(nl.input.parts[i])) refuse(b.nl, "its first three inputs are not the nodes z_t, r_t and hpart_t");
      const int z_t = nl.input.parts[0].terms[0].node, r_t = nl.input.parts[1].terms[0].node;
      b.hp = nl.input.parts[2].terms[0].node;
      b.delay = recurrent_part(b.nl, nl.input.parts[3], &b.sc);
      int s_nl = b.sc;
      if (proj) {
        const int d2 = recurrent_part(b.nl, nl.input.parts[4], &s_nl);
        if (d2 != b.delay) refuse(b.nl, "two different delays in one block, " + std::to_string(d2) + " and " + std::to_string(b.delay));
        if (!range_of(b.sc, b.nl, C, C)) refuse(b.sc, "the cell state is not the second cell-dim columns of the nonlinearity");
      }
      b.tr = b.sr = s_nl;
      if (comp_type(b.tr) != "BackpropTruncationComponent") refuse(b.tr, "the recurrent state does not come through a BackpropTruncationComponent");
      // a gate: [DropoutComponent over] a SigmoidComponent over an affine over Append(x, IfDefined(Offset(s_t, -d)))
      auto gate = [&](int g, int rows, const char *rows_name, int *drop, int *sig, int *aff) {
        *drop = -1;
        if (comp_type(g) == "DropoutComponent") {
          *drop = g;
          g = only_input(g);
          if (g < 0) refuse(*drop, "the dropout's input is not one node");
        }
        if (comp_type(g) != "SigmoidComponent") refuse(g, "the gate is not a SigmoidComponent node [behind a DropoutComponent]");
        *sig = g;
        const int a = only_input(g);
        if (a < 0 || !is_affine(a)) refuse(g, "the sigmoid's input is not an affine component node");
        *aff = a;
        const NnetNode &an = nodes[a];
        if (an.input.parts.size() < 2) refuse(a, "its input is not Append(x, IfDefined(Offset(s_t, -delay)))");
        int state = -1;
        const int d2 = recurrent_part(a, an.input.parts.back(), &state);
        if (d2 != b.delay) refuse(a, "two different delays in one block, " + std::to_string(d2) + " and " + std::to_string(b.delay));
        if (state != b.tr) refuse(a, "the gate and the nonlinearity read different recurrent states, " + nodes[state].name + " and " + nodes[b.tr].name);
        if (an.dim != rows) refuse(a, "the gate's affine has " + std::to_string(an.dim) + " rows, not the " + rows_name + " " + std::to_string(rows));
      };
      gate(z_t, C, "cell's dim", &b.zd, &b.zs, &b.wa);
      gate(r_t, R, "recurrent dim", &b.od, &b.os, &b.wo);
      if ((b.zd >= 0) != (b.od >= 0)) refuse(b.zd >= 0 ? b.zd : b.od, "only one of the two gates has a DropoutComponent");
      // the state: s_t from W_y's first columns [through a NormalizeComponent]; without a projection from the nonlinearity's c columns
      int src = only_input(b.tr);
      if (proj) {
        if (src >= 0 && comp_type(src) == "NormalizeComponent") {
          b.nm = src;
          const Component &nmc = net.components[nodes[b.nm].component];
          if (nmc.f.count("<AddLogStddev>") && nmc.f.at("<AddLogStddev>")[0] != 0.0) refuse(b.nm, "a NormalizeComponent with add-log-stddev=true is not supported");
          if (nmc.f.count("<BlockDim>") && nmc.Int("<BlockDim>") != (nmc.i.count("<InputDim>") ? nmc.Int("<InputDim>") : nmc.Int("<Dim>")))
            refuse(b.nm, "a NormalizeComponent with block-dim is not supported");
          src = only_input(b.nm);
        }
        if (src < 0 || nodes[src].kind != NnetNode::kDimRange) refuse(b.tr, "the recurrent state is not a dim-range of W_y's node [through a NormalizeComponent]");
        b.sp = src;
        b.wy = nodes[b.sp].range_node;
        if (!is_affine(b.wy) || !range_of(b.sp, b.wy, 0, R) || nodes[b.tr].dim != R) refuse(b.sp, "the recurrent state is not the first recurrent-dim columns of an affine component node");
        if (only_input(b.wy) != b.sc) refuse(b.wy, "W_y's input is not the cell state " + nodes[b.sc].name);
      } else {
        if (src < 0 || !range_of(src, b.nl, C, C) || nodes[b.tr].dim != C) refuse(b.tr, "without a projection the recurrent state is not the second cell-dim columns of the nonlinearity");
        b.sc = src;      // (y_t: the layer's output)
      }
      // the feed-forward input: the same descriptor in front of both gates and under hpart_t
      const NnetNode &wz = nodes[b.wa], &wr = nodes[b.wo], &hp = nodes[b.hp];
      b.x_parts.assign(wz.input.parts.begin(), wz.input.parts.end() - 1);
      if (!same_parts(wr.input.parts, wr.input.parts.size() - 1, b.x_parts)) refuse(b.wo, "the two gates do not read the same feed-forward input");
      if (!is_affine(b.hp) || !same_parts(hp.input.parts, hp.input.parts.size(), b.x_parts))
        refuse(b.hp, "hpart_t is not an affine component node over the gates' feed-forward input");
      for (auto &p : b.x_parts) for (auto &t : p.terms) if (in_scc(t.node)) refuse(b.wa, "its feed-forward input reads " + nodes[t.node].name + ", a node of the cycle");
      b.members = {b.wa, b.wo, b.zs, b.os, b.nl, b.sc, b.tr};
      for (int n : {b.zd, b.od, b.nm, b.wy, b.sp}) if (n >= 0) b.members.push_back(n);
      std::sort(b.members.begin(), b.members.end());
      if (std::adjacent_find(b.members.begin(), b.members.end()) != b.members.end()) refuse(b.nl, "a node has two roles in the block");
      for (int n : scc) if (!std::binary_search(b.members.begin(), b.members.end(), n)) refuse(n, "the node is part of the cycle but not of such a block");
      for (int n : b.members) if (!in_scc(n)) refuse(n, "the node is not part of the cycle");
      if (in_scc(b.hp) || (*block_of)[b.hp] >= 0) refuse(b.hp, "hpart_t is part of a cycle");
      // dims against the weights
      int x_dim = 0;
      for (auto &p : b.x_parts) x_dim += p.dim;
      for (int a : {b.wa, b.wo}) {
        const MatF &W = net.components[nodes[a].component].m.at("<LinearParams>");
        if (W.cols != x_dim + R)
          refuse(a, "its weights are " + std::to_string(W.rows) + " x " + std::to_string(W.cols) + ", the block needs the feed-forward input's " +
                        std::to_string(x_dim) + " + the recurrent input's " + std::to_string(R) + " columns");
      }
      const MatF &Wh = net.components[hp.component].m.at("<LinearParams>");
      if (Wh.rows != C || Wh.cols != x_dim) refuse(b.hp, "its weights are " + std::to_string(Wh.rows) + " x " + std::to_string(Wh.cols) + ", not cell-dim x the feed-forward input's dim");
      if (proj) {
        const MatF &Wy = net.components[nodes[b.wy].component].m.at("<LinearParams>");
        if (Wy.cols != C || Wy.rows < R) refuse(b.wy, "W_y is " + std::to_string(Wy.rows) + " x " + std::to_string(Wy.cols) + ", the block needs cell-dim columns and at least the recurrent dim's rows");
      }
      // only what has a buffer may be read from outside the block: the nonlinearity, c_t, W_y's node, its dim-range and the state
      for (int n = 0; n < N; n++) {
        if (std::binary_search(b.members.begin(), b.members.end(), n) || index[n] < 0) continue;
        std::vector<int> d;
        deps(n, &d);
        for (int m : d)
          if (m == b.wa || m == b.wo || m == b.zs || m == b.os || m == b.zd || m == b.od || m == b.nm || (m == b.hp && n != b.nl))
            refuse(m, "the node is read from outside the block, by " + nodes[n].name);
      }
      b.members.push_back(b.hp);
      std::sort(b.members.begin(), b.members.end());
      for (int n : b.members) (*block_of)[n] = (int)blocks->size();
      blocks->push_back(std::move(b));
      continue;
    }
    if (gru_cycle) {
      b.gru = true;
      b.nl = -1;
      for (int n : scc)
        if (comp_type(n) == "OutputGruNonlinearityComponent") {
          if (b.nl >= 0) refuse(n, "a second OutputGruNonlinearityComponent in one cycle");
          b.nl = n;
        }
      // the nonlinearity: Append(z_t, hpart_t, IfDefined(Offset(c_t, -d)))
      const NnetNode &nl = nodes[b.nl];
      const int C = b.cell = nl.dim / 2;
      if (nl.input.parts.size() != 3) refuse(b.nl, "its input is not Append(z_t, hpart_t, IfDefined(Offset(c_t, -delay)))");
      for (auto &p : nl.input.parts) if (p.dim != C) refuse(b.nl, "its three inputs are not of the cell's dim");
      if (!plain_part(nl.input.parts[0]) || !plain_part(nl.input.parts[1])) refuse(b.nl, "its first two inputs are not the nodes z_t and hpart_t");
      const int z_t = nl.input.parts[0].terms[0].node;
      b.hp = nl.input.parts[1].terms[0].node;
      b.delay = recurrent_part(b.nl, nl.input.parts[2], &b.sc);
      if (!range_of(b.sc, b.nl, C, C)) refuse(b.sc, "the cell state is not the second cell-dim columns of the nonlinearity");
      // a gate: [DropoutComponent over] a SigmoidComponent over an affine over Append(x, IfDefined(Offset(s_t, -d)))
      auto gate = [&](int g, int *drop, int *sig, int *aff, int *state) {
        *drop = -1;
        if (comp_type(g) == "DropoutComponent") {
          *drop = g;
          g = only_input(g);
          if (g < 0) refuse(*drop, "the dropout's input is not one node");
        }
        if (comp_type(g) != "SigmoidComponent") refuse(g, "the gate is not a SigmoidComponent node [behind a DropoutComponent]");
        *sig = g;
        const int a = only_input(g);
        if (a < 0 || !is_affine(a)) refuse(g, "the sigmoid's input is not an affine component node");
        *aff = a;
        const NnetNode &an = nodes[a];
        if (an.input.parts.size() < 2) refuse(a, "its input is not Append(x, IfDefined(Offset(s_t, -delay)))");
        const int d2 = recurrent_part(a, an.input.parts.back(), state);
        if (d2 != b.delay) refuse(a, "two different delays in one block, " + std::to_string(d2) + " and " + std::to_string(b.delay));
        if (an.dim != C) refuse(a, "the gate's affine has " + std::to_string(an.dim) + " rows, not the cell's dim " + std::to_string(C));
      };
      int s_z = -1, s_o = -1;
      gate(z_t, &b.zd, &b.zs, &b.wa, &s_z);
      // the product Append(c_t, o_t), W_y over it, the state from W_y's first columns
      b.tr = b.sr = s_z;
      if (comp_type(b.tr) != "BackpropTruncationComponent") refuse(b.tr, "the recurrent state does not come through a BackpropTruncationComponent");
      int src = only_input(b.tr);
      if (src >= 0 && comp_type(src) == "NormalizeComponent") {
        b.nm = src;
        const Component &nc = net.components[nodes[b.nm].component];
        if (nc.f.count("<AddLogStddev>") && nc.f.at("<AddLogStddev>")[0] != 0.0) refuse(b.nm, "a NormalizeComponent with add-log-stddev=true is not supported");
        if (nc.f.count("<BlockDim>") && nc.Int("<BlockDim>") != (nc.i.count("<InputDim>") ? nc.Int("<InputDim>") : nc.Int("<Dim>")))
          refuse(b.nm, "a NormalizeComponent with block-dim is not supported");
        src = only_input(b.nm);
      }
      if (src < 0 || nodes[src].kind != NnetNode::kDimRange) refuse(b.tr, "the recurrent state is not a dim-range of W_y's node [through a NormalizeComponent]");
      b.sp = src;
      b.wy = nodes[b.sp].range_node;
      b.rec_dim = nodes[b.sp].dim;
      if (!is_affine(b.wy) || !range_of(b.sp, b.wy, 0, b.rec_dim) || nodes[b.tr].dim != b.rec_dim)
        refuse(b.sp, "the recurrent state is not the first columns of an affine component node");
      b.cd = only_input(b.wy);
      if (b.cd < 0 || comp_type(b.cd) != "ElementwiseProductComponent") refuse(b.wy, "W_y's input is not an ElementwiseProductComponent node");
      const NnetNode &cd = nodes[b.cd];
      if (cd.input.parts.size() != 2 || !plain_part(cd.input.parts[0]) || !plain_part(cd.input.parts[1]) || cd.input.parts[0].terms[0].node != b.sc ||
          cd.input.parts[1].dim != C || cd.dim != C)
        refuse(b.cd, "the product's input is not Append(c_t, o_t)");
      gate(cd.input.parts[1].terms[0].node, &b.od, &b.os, &b.wo, &s_o);
      if (s_o != b.tr) refuse(b.wo, "the two gates read different recurrent states, " + nodes[s_z].name + " and " + nodes[s_o].name);
      if ((b.zd >= 0) != (b.od >= 0) || (b.zd >= 0 && nodes[b.zd].component != nodes[b.od].component))
        refuse(b.zd >= 0 ? b.zd : b.od, "the two gates do not share one DropoutComponent");
      // the feed-forward input: the same descriptor in front of both gates and under hpart_t
      const NnetNode &wz = nodes[b.wa], &wo = nodes[b.wo], &hp = nodes[b.hp];
      b.x_parts.assign(wz.input.parts.begin(), wz.input.parts.end() - 1);
      if (!same_parts(wo.input.parts, wo.input.parts.size() - 1, b.x_parts)) refuse(b.wo, "the two gates do not read the same feed-forward input");
      if (!is_affine(b.hp) || !same_parts(hp.input.parts, hp.input.parts.size(), b.x_parts))
        refuse(b.hp, "hpart_t is not an affine component node over the gates' feed-forward input");
      for (auto &p : b.x_parts) for (auto &t : p.terms) if (in_scc(t.node)) refuse(b.wa, "its feed-forward input reads " + nodes[t.node].name + ", a node of the cycle");
      b.members = {b.wa, b.wo, b.zs, b.os, b.nl, b.sc, b.cd, b.wy, b.sp, b.tr};
      for (int n : {b.zd, b.od, b.nm}) if (n >= 0) b.members.push_back(n);
      std::sort(b.members.begin(), b.members.end());
      if (std::adjacent_find(b.members.begin(), b.members.end()) != b.members.end()) refuse(b.nl, "a node has two roles in the block");
      for (int n : scc) if (!std::binary_search(b.members.begin(), b.members.end(), n)) refuse(n, "the node is part of the cycle but not of such a block");
      for (int n : b.members) if (!in_scc(n)) refuse(n, "the node is not part of the cycle");
      if (in_scc(b.hp) || (*block_of)[b.hp] >= 0) refuse(b.hp, "hpart_t is part of a cycle");
      // dims against the weights
      int x_dim = 0;
      for (auto &p : b.x_parts) x_dim += p.dim;
      const int R = b.rec_dim;
      for (int a : {b.wa, b.wo}) {
        const MatF &W = net.components[nodes[a].component].m.at("<LinearParams>");
        if (W.rows != C || W.cols != x_dim + R)
          refuse(a, "its weights are " + std::to_string(W.rows) + " x " + std::to_string(W.cols) + ", the block needs cell-dim rows and the feed-forward input's " +
                        std::to_string(x_dim) + " + the recurrent input's " + std::to_string(R) + " columns");
      }
      const MatF &Wh = net.components[hp.component].m.at("<LinearParams>"), &Wy = net.components[nodes[b.wy].component].m.at("<LinearParams>");
      if (Wh.rows != C || Wh.cols != x_dim) refuse(b.hp, "its weights are " + std::to_string(Wh.rows) + " x " + std::to_string(Wh.cols) + ", not cell-dim x the feed-forward input's dim");
      if (Wy.cols != C || Wy.rows < R) refuse(b.wy, "W_y is " + std::to_string(Wy.rows) + " x " + std::to_string(Wy.cols) + ", the block needs cell-dim columns and at least the recurrent dim's rows");
      if (nl.input.dim != 3 * C) refuse(b.nl, "its input dim is not 3 x cell-dim");
      // only what has a buffer may be read from outside the block: the nonlinearity, c_t, W_y's node, its dim-range and the state
      for (int n = 0; n < N; n++) {
        if (std::binary_search(b.members.begin(), b.members.end(), n) || index[n] < 0) continue;
        std::vector<int> d;
        deps(n, &d);
        for (int m : d)
          if (m == b.wa || m == b.wo || m == b.zs || m == b.os || m == b.zd || m == b.od || m == b.cd || m == b.nm || (m == b.hp && n != b.nl))
            refuse(m, "the node is read from outside the block, by " + nodes[n].name);
      }
      b.members.push_back(b.hp);
      std::sort(b.members.begin(), b.members.end());
      for (int n : b.members) (*block_of)[n] = (int)blocks->size();
      blocks->push_back(std::move(b));
      continue;
    }
    // the nonlinearity: Append(W_all, IfDefined(Offset(c_trunc, -d)) [, dropout_mask])
    const NnetNode &nl = nodes[b.nl];
    const int C = b.cell = nl.dim / 2;
    if (nl.input.parts.size() != 2 && nl.input.parts.size() != 3) refuse(b.nl, "its input is not Append(W_all, IfDefined(Offset(c_trunc, -delay)) [, dropout_mask])");
    if (!plain_part(nl.input.parts[0]) || nl.input.parts[0].dim != 4 * C) refuse(b.nl, "its first input is not a node of dim 4 x cell-dim");
    b.wa = nl.input.parts[0].terms[0].node;
    if (nl.input.parts[1].dim != C) refuse(b.nl, "its second input is not of the cell's dim");
    b.delay = recurrent_part(b.nl, nl.input.parts[1], &b.sc);
    if (nl.input.parts.size() == 3) {
      if (!plain_part(nl.input.parts[2]) || nl.input.parts[2].dim != 3 || comp_type(nl.input.parts[2].terms[0].node) != "DropoutMaskComponent")
        refuse(b.nl, "its third input is not a 3-column DropoutMaskComponent node");
      b.dm = nl.input.parts[2].terms[0].node;
      const Component &dm = net.components[nodes[b.dm].component];
      // test mode (the binaries set it): ones with dropout-proportion 0 or <Continuous>, else 1 - proportion (nnet-general-component.cc:1429-1449)
      const bool continuous = dm.b.count("<Continuous>") != 0;
      if (!continuous && dm.f.count("<DropoutProportion>") && dm.f.at("<DropoutProportion>")[0] != 0.0)
        refuse(b.dm, "a non-continuous dropout mask with dropout-proportion " + std::to_string(dm.f.at("<DropoutProportion>")[0]) + " is not all ones in test mode");
    }
    if (in_scc(b.wa) && comp_type(b.wa) == "ScaleAndOffsetComponent") {
      // ---- the cell behind a bottleneck (xconfig/lstm.py: XconfigLstmbLayer :860-950): the nonlinearity's first input is W_all_b_so, a
      // ScaleAndOffsetComponent over the LinearComponent W_all_b over the LinearComponent W_all_a, which reads
      // Append(x ..., IfDefined(Offset([Scale(s,)] m_trunc, -d)))
      b.lstmb = true;
      b.so = b.wa;
      if (b.dm >= 0) refuse(b.nl, "an lstmb-layer block's nonlinearity takes no third input, but this one reads the dropout mask " + nodes[b.dm].name);
      const Component &so = net.components[nodes[b.so].component];
      {
        auto sit = so.v.find("<Scales>"), oit = so.v.find("<Offsets>");
        if (nodes[b.so].dim != 4 * C || sit == so.v.end() || oit == so.v.end() || (int)sit->second.size() != 4 * C || (int)oit->second.size() != 4 * C)
          refuse(b.so, "the ScaleAndOffsetComponent in front of the nonlinearity does not have <Scales> and <Offsets> vectors of 4 x cell-dim = " + std::to_string(4 * C) +
                           " elements (its block form is not supported inside a recurrent block)");
      }
      b.wb = only_input(b.so);
      if (b.wb < 0 || !in_scc(b.wb) || comp_type(b.wb) != "LinearComponent") refuse(b.so, "its input is not a LinearComponent node of the cycle (W_all_b)");
      b.wa = only_input(b.wb);
      if (b.wa < 0 || !in_scc(b.wa) || comp_type(b.wa) != "LinearComponent") refuse(b.wb, "its input is not a LinearComponent node of the cycle (W_all_a)");
      const NnetNode &wa = nodes[b.wa];
      if (wa.input.parts.size() < 2) refuse(b.wa, "its input is not Append(x, IfDefined(Offset(m_trunc, -delay)))");
      const int d2 = recurrent_part(b.wa, wa.input.parts.back(), &b.sr, &b.self_scale);
      if (d2 != b.delay) refuse(b.wa, "two different delays in one block, " + std::to_string(d2) + " and " + std::to_string(b.delay));
      b.rec_dim = wa.input.parts.back().dim;
      b.x_parts.assign(wa.input.parts.begin(), wa.input.parts.end() - 1);
      for (auto &p : b.x_parts) for (auto &t : p.terms) if (in_scc(t.node)) refuse(b.wa, "its feed-forward input reads " + nodes[t.node].name + ", a node of the cycle");
      // the state: the two column ranges of one BackpropTruncationComponent node over the nonlinearity
      if (nodes[b.sc].kind != NnetNode::kDimRange) refuse(b.sc, "the cell state is not a dim-range of a BackpropTruncationComponent node");
      b.tr = nodes[b.sc].range_node;
      if (comp_type(b.tr) != "BackpropTruncationComponent") refuse(b.tr, "the state does not come through a BackpropTruncationComponent");
      if (only_input(b.tr) != b.nl) refuse(b.tr, "its input is not the nonlinearity: an lstmb-layer block has no projection");
      if (b.rec_dim != C || !range_of(b.sc, b.tr, 0, C) || !range_of(b.sr, b.tr, C, C) || nodes[b.tr].dim != 2 * C)
        refuse(b.tr, "c_trunc and m_trunc are not the two cell-dim column ranges of one BackpropTruncationComponent node");
      b.members = {b.wa, b.wb, b.so, b.nl, b.tr, b.sc, b.sr};
      std::sort(b.members.begin(), b.members.end());
      if (std::adjacent_find(b.members.begin(), b.members.end()) != b.members.end()) refuse(b.nl, "a node has two roles in the block");
      for (int n : scc) if (!std::binary_search(b.members.begin(), b.members.end(), n)) refuse(n, "the node is part of the cycle but not of such a block");
      for (int n : b.members) if (!in_scc(n)) refuse(n, "the node is not part of the cycle");
      auto params_of = [&](int n) -> const MatF * { const Component &c = net.components[nodes[n].component]; auto it = c.m.find("<Params>"); return it == c.m.end() ? nullptr : &it->second; };
      const MatF *Wa = params_of(b.wa), *Wb = params_of(b.wb);
      int x_dim = 0;
      for (auto &p : b.x_parts) x_dim += p.dim;
      if (!Wa || Wa->rows <= 0 || Wa->cols != x_dim + C)
        refuse(b.wa, "W_all_a is " + std::to_string(Wa ? Wa->rows : 0) + " x " + std::to_string(Wa ? Wa->cols : 0) + ", the block needs the feed-forward input's " + std::to_string(x_dim) +
                         " + the cell's " + std::to_string(C) + " columns");
      if (!Wb || Wb->rows != 4 * C || Wb->cols != Wa->rows)
        refuse(b.wb, "W_all_b is " + std::to_string(Wb ? Wb->rows : 0) + " x " + std::to_string(Wb ? Wb->cols : 0) + ", the block needs 4 x cell-dim rows and the bottleneck's " +
                         std::to_string(Wa->rows) + " columns");
      if (nl.input.dim != 5 * C) refuse(b.nl, "its input dim is not 5 x cell-dim");
      // only m, the second cell-dim columns of the nonlinearity, may be read from outside the block
      for (int n = 0; n < N; n++) {
        if (std::binary_search(b.members.begin(), b.members.end(), n) || index[n] < 0) continue;
        std::vector<int> d;
        deps(n, &d);
        for (int m : d)
          if (std::binary_search(b.members.begin(), b.members.end(), m) && !(m == b.nl && range_of(n, b.nl, C, C)))
            refuse(m, "the node is read from outside the block, by " + nodes[n].name);
      }
      for (int n : b.members) (*block_of)[n] = (int)blocks->size();
      blocks->push_back(std::move(b));
      continue;
    }
    // W_all: Append(x ..., IfDefined(Offset(r_trunc, -d)))
    const std::string wt = comp_type(b.wa);
    if (!in_scc(b.wa) || (wt != "AffineComponent" && wt != "NaturalGradientAffineComponent")) refuse(b.wa, "the nonlinearity's first input is not an affine component node of the cycle");
    const NnetNode &wa = nodes[b.wa];
    if (wa.input.parts.size() < 2) refuse(b.wa, "its input is not Append(x, IfDefined(Offset(r_trunc, -delay)))");
    const int d2 = recurrent_part(b.wa, wa.input.parts.back(), &b.sr);
    if (d2 != b.delay) refuse(b.wa, "two different delays in one block, " + std::to_string(d2) + " and " + std::to_string(b.delay));
    b.rec_dim = wa.input.parts.back().dim;
    b.x_parts.assign(wa.input.parts.begin(), wa.input.parts.end() - 1);
    for (auto &p : b.x_parts) for (auto &t : p.terms) if (in_scc(t.node)) refuse(b.wa, "its feed-forward input reads " + nodes[t.node].name + ", a node of the cycle");
    // the state: dim-ranges of one BackpropTruncationComponent node
    if (nodes[b.sc].kind != NnetNode::kDimRange) refuse(b.sc, "the cell state is not a dim-range of a BackpropTruncationComponent node");
    b.tr = nodes[b.sc].range_node;
    if (comp_type(b.tr) != "BackpropTruncationComponent") refuse(b.tr, "the state does not come through a BackpropTruncationComponent");
    if (!range_of(b.sc, b.tr, 0, C) || !range_of(b.sr, b.tr, C, b.rec_dim) || nodes[b.tr].dim != C + b.rec_dim)
      refuse(b.tr, "c_trunc and r_trunc / m_trunc are not the two column ranges of one BackpropTruncationComponent node");
    const NnetNode &tr = nodes[b.tr];
    if (tr.input.parts.size() == 1 && plain_part(tr.input.parts[0]) && tr.input.parts[0].terms[0].node == b.nl) {
      if (b.rec_dim != C) refuse(b.tr, "without a projection the recurrent input is m, of the cell's dim");
      b.members = {b.wa, b.nl, b.tr, b.sc, b.sr};
    } else {
      if (tr.input.parts.size() != 2 || !plain_part(tr.input.parts[0]) || !plain_part(tr.input.parts[1])) refuse(b.tr, "its input is neither the nonlinearity nor Append(c, r)");
      b.c = tr.input.parts[0].terms[0].node;
      b.r = tr.input.parts[1].terms[0].node;
      if (!range_of(b.c, b.nl, 0, C)) refuse(b.c, "not the first cell-dim columns of the nonlinearity");
      if (nodes[b.r].kind != NnetNode::kDimRange) refuse(b.r, "not a dim-range of the projection");
      b.rp = nodes[b.r].range_node;
      const std::string rt = comp_type(b.rp);
      if ((rt != "AffineComponent" && rt != "NaturalGradientAffineComponent") || !range_of(b.r, b.rp, 0, b.rec_dim) || nodes[b.rp].dim < b.rec_dim)
        refuse(b.rp, "r is not the first columns of an affine projection");
      const NnetNode &rp = nodes[b.rp];
      if (rp.input.parts.size() != 1 || !plain_part(rp.input.parts[0])) refuse(b.rp, "the projection's input is not m");
      b.m = rp.input.parts[0].terms[0].node;
      if (!range_of(b.m, b.nl, C, C)) refuse(b.m, "not the second cell-dim columns of the nonlinearity");
      if (net.components[rp.component].m.at("<LinearParams>").cols != C) refuse(b.rp, "the projection's input dim is not the cell's");
      b.members = {b.wa, b.nl, b.tr, b.sc, b.sr, b.c, b.m, b.rp, b.r};
    }
    std::sort(b.members.begin(), b.members.end());
    if (std::adjacent_find(b.members.begin(), b.members.end()) != b.members.end()) refuse(b.nl, "a node has two roles in the block");
    for (int n : scc) if (!std::binary_search(b.members.begin(), b.members.end(), n)) refuse(n, "the node is part of the cycle but not of such a block");
    for (int n : b.members) if (!in_scc(n)) refuse(n, "the node is not part of the cycle");
    const MatF &W = net.components[wa.component].m.at("<LinearParams>");
    if (W.rows != 4 * C || W.cols <= b.rec_dim) refuse(b.wa, "W_all is " + std::to_string(W.rows) + " x " + std::to_string(W.cols) + ", the block needs 4 x cell-dim rows and more columns than the recurrent input has");
    if (nl.input.dim != 5 * C + (b.dm >= 0 ? 3 : 0)) refuse(b.nl, "its input dim is not 5 x cell-dim (+ 3 with a dropout mask)");
    for (int n : b.members) (*block_of)[n] = (int)blocks->size();
    blocks->push_back(std::move(b));
  }
  // a Const() term has no node: it is known only as the 1 of the (1 - z_t) in y1_t of a composed GRU block
  for (int n = 0; n < N; n++) {
    if (index[n] < 0) continue;
    bool konst = false;
    for (auto &p : nodes[n].input.parts) for (auto &t : p.terms) konst = konst || t.konst;
    if (konst && !((*block_of)[n] >= 0 && (*blocks)[(*block_of)[n]].gruc && (*blocks)[(*block_of)[n]].y1 == n))
      Fail("nnet3: Const() in the input of node " + nodes[n].name + " is supported only as the Sum(Scale(-1.0, z_t), Const(1.0, cell-dim)) of a gru-layer / pgru-layer / "
           "norm-pgru-layer / opgru-layer / norm-opgru-layer block");
  }
  // IfDefined() outside a cycle: the reference leaves the term out of the network's context and fills the rows it then cannot compute
  // (the first frames of an utterance for Offset(x, -2)) with zeros; the feed-forward lowering has no optional inputs
  for (int n = 0; n < N; n++) {
    if (index[n] < 0 || (*block_of)[n] >= 0) continue;
    for (auto &p : nodes[n].input.parts)
      for (auto &t : p.terms)
        if (t.optional)
          Fail("nnet3: IfDefined() in the input of node " + nodes[n].name + " (over " + nodes[t.node].name + ") is supported only as the recurrent connection of a "
               "recurrent block: outside a cycle the reference zero-fills the rows it cannot compute, which the feed-forward path does not do");
  }
  // a block whose feed-forward input reads another block's state at a future time would need that block's rows before they exist
  for (const BlockNodes &b : *blocks)
    for (auto &p : b.x_parts)
      for (auto &t : p.terms)
        for (const BlockNodes &o : *blocks)
          if ((t.node == o.tr || t.node == o.sc || t.node == o.sr) && t.offset > 0)
            Fail("nnet3: recurrent networks are supported only as fast-lstmp-layer / fast-lstm-layer blocks (cycle at node " + nodes[b.wa].name + ": it reads the state " +
                 nodes[t.node].name + " of another block at a future time, offset " + std::to_string(t.offset) + ")");
}

void CheckRecurrence(const Nnet &net) {
  std::vector<BlockNodes> blocks;
  std::vector<int> block_of;
  const int out = net.FindNode("output");
  if (out >= 0) FindBlocks(net, out, &blocks, &block_of);
}
}  // namespace

void Nnet::Compile() {
  int out_node = FindNode("output");
  int in_node = FindNode("input"), iv_node = FindNode("ivector");
  const int N = (int)nodes.size();
  // recurrent blocks: the cycles of the node graph, each of which has to be what fast-lstmp-layer / fast-lstm-layer, lstmp-layer / lstm-layer,
  // fast-opgru-layer / fast-norm-opgru-layer, fast-pgru-layer / fast-norm-pgru-layer / fast-gru-layer or gru-layer / pgru-layer /
  // norm-pgru-layer / opgru-layer / norm-opgru-layer emit
  std::vector<BlockNodes> blocks;
  std::vector<int> block_of(N, -1);
  FindBlocks(*this, out_node, &blocks, &block_of);
  recurrent = !blocks.empty();
  // reachable set + topological order (DFS post-order); a block is one unit, placed where its affine node W_all would be
  std::vector<int> order, state(N, 0);
  std::function<void(int)> visit = [&](int n) {
    if (state[n] == 2) return;
    if (state[n] == 1) Fail("nnet3: internal error, a cycle outside the recurrent blocks (node " + nodes[n].name + ")");
    if (block_of[n] >= 0) {
      const BlockNodes &b = blocks[block_of[n]];
      for (int m : b.members) state[m] = 1;
      for (auto &p : b.x_parts) for (auto &t : p.terms) visit(t.node);
      for (int m : b.members) state[m] = 2;
      if (b.dm >= 0) state[b.dm] = 2;
      order.push_back(b.wa);
      return;
    }
    state[n] = 1;
    const NnetNode &nd = nodes[n];
    if (nd.kind == NnetNode::kComponent && components[nd.component].type == "DropoutMaskComponent")
      Fail("nnet3: DropoutMaskComponent node " + nd.name + " is supported only as the dropout mask of an LstmNonlinearityComponent inside a recurrent block");
    if (nd.kind == NnetNode::kDimRange) visit(nd.range_node);
    for (auto &p : nd.input.parts) for (auto &t : p.terms) visit(t.node);
    state[n] = 2;
    order.push_back(n);
  };
  visit(out_node);
  // consumer counts (only "plain" uses allow fusing)
  std::vector<int> consumers(N, 0);
  for (int n : order) {
    const NnetNode &nd = nodes[n];
    if (nd.kind == NnetNode::kDimRange) consumers[nd.range_node] += 2;  // never fuse through a dim-range
    for (auto &p : nd.input.parts) for (auto &t : p.terms) consumers[t.node]++;
  }
  // Tdnn components contribute their own time offsets on top of the descriptor's.
  auto tdnn_offsets = [&](const NnetNode &nd) -> std::vector<int> {
    if (nd.kind == NnetNode::kComponent && components[nd.component].type == "TdnnComponent") {
      const auto &c = components[nd.component];
      auto it = c.iv.find("<TimeOffsets>");
      if (it == c.iv.end() || it->second.empty()) Fail("nnet3: TdnnComponent without <TimeOffsets>");
      return std::vector<int>(it->second.begin(), it->second.end());
    }
    if (nd.kind == NnetNode::kComponent && components[nd.component].type == "TimeHeightConvolutionComponent")
      return ReadConvGeom(components[nd.component], component_names[nd.component]).time_offsets;
    if (nd.kind == NnetNode::kComponent && components[nd.component].type == "RestrictedAttentionComponent") {
      const AttentionGeom g = ReadAttentionGeom(components[nd.component], component_names[nd.component], nd.name);
      std::vector<int> offs;
      for (int o = 0; o < g.Context(); o++) offs.push_back(g.TimeOffset(o));
      return offs;
    }
    return {0};
  };
  // required extension per node: rows t in [-lext, T+rext)
  // A recurrent block's rows: to the right what its readers need; to the left, where `avail` is given, every row that is
  // computable from the input the first chunk requests (t >= -left_context) -- the computation graph builder computes every
  // cell that is computable and reachable, so a chain t, t - d, ... starts at the first t' of its residue class at which the
  // block's feed-forward input exists, and IfDefined supplies zeros before that.  The recurrent connection itself asks for
  // nothing (ComputeSimpleNnetContext ignores the optional dependency).
  std::vector<int> lext, rext;
  auto extents = [&](const std::vector<int> *avail) {
    lext.assign(N, 0);
    rext.assign(N, 0);
    for (auto it = order.rbegin(); it != order.rend(); ++it) {
      int n = *it;
      const NnetNode &nd = nodes[n];
      if (nd.kind == NnetNode::kDimRange) {
        lext[nd.range_node] = std::max(lext[nd.range_node], lext[n]);
        rext[nd.range_node] = std::max(rext[nd.range_node], rext[n]);
        continue;
      }
      if (block_of[n] >= 0) {
        BlockNodes &b = blocks[block_of[n]];
        int l = 0, r = 0;
        for (int m : b.members) { l = std::max(l, lext[m]); r = std::max(r, rext[m]); }
        b.need_lext = l;
        if (avail) l = std::max(l, (*avail)[b.wa]);
        for (int m : b.members) { lext[m] = l; rext[m] = r; }
        for (auto &p : b.x_parts)
          for (auto &t : p.terms) {
            if (t.const_t) continue;
            lext[t.node] = std::max(lext[t.node], l - t.offset);
            rext[t.node] = std::max(rext[t.node], r + t.offset);
          }
        continue;
      }
      std::vector<int> toffs = tdnn_offsets(nd);
      for (auto &p : nd.input.parts)
        for (auto &t : p.terms) {
          if (t.const_t) continue;
          for (int o2 : toffs) {
            int o = t.offset + o2;
            lext[t.node] = std::max(lext[t.node], lext[n] - o);
            rext[t.node] = std::max(rext[t.node], rext[n] + o);
          }
        }
    }
  };
  extents(nullptr);
  left_context = lext[in_node];
  right_context = rext[in_node];
  if (recurrent) {
    // avail[n]: node n is computable for t >= -avail[n] when the input is there for t >= -left_context
    const int kFree = 1 << 28;
    std::vector<int> avail(N, kFree);
    avail[in_node] = left_context;
    for (int n : order) {
      const NnetNode &nd = nodes[n];
      if (nd.kind == NnetNode::kInput) continue;
      if (nd.kind == NnetNode::kDimRange) { avail[n] = avail[nd.range_node]; continue; }
      int a = kFree;
      if (block_of[n] >= 0) {
        const BlockNodes &b = blocks[block_of[n]];
        for (auto &p : b.x_parts) for (auto &t : p.terms) if (!t.const_t) a = std::min(a, avail[t.node] + t.offset);
        if (a >= kFree / 2) Fail("nnet3: recurrent block at node " + nd.name + " has no input that depends on time");
        for (int m : b.members) avail[m] = a;
        continue;
      }
      for (int o2 : tdnn_offsets(nd))
        for (auto &p : nd.input.parts) for (auto &t : p.terms) if (!t.const_t) a = std::min(a, avail[t.node] + t.offset + o2);
      avail[n] = a;
    }
    extents(&avail);
    if (lext[in_node] != left_context || rext[in_node] != right_context)
      Fail("nnet3: internal error, the rows of the recurrent blocks reach beyond the network's context");
  }

  // buffer assignment
  std::vector<int> node_buf(N, -1), node_col(N, 0);
  std::vector<int> node_op(N, -1);     // op producing the node's buffer (for fusing)
  ops.clear();
  bufs.clear();
  auto new_buf = [&](int dim, int l, int r) { BufferInfo b; b.dim = dim; b.lext = l; b.rext = r; bufs.push_back(b); return (int)bufs.size() - 1; };
  input_buf = new_buf(nodes[in_node].dim, lext[in_node], rext[in_node]);
  bufs[input_buf].is_input = true;
  node_buf[in_node] = input_buf;
  if (iv_node >= 0) node_buf[iv_node] = -2;  // special: iVector rows

  // materialise one descriptor part (a Sum of terms) as an eltwise op if it is not a plain reference
  auto term_src = [&](const DescTerm &t, int *buf, int *col) {
    if (node_buf[t.node] == -1) Fail("nnet3: internal error, node " + nodes[t.node].name + " used before it was computed");
    *buf = node_buf[t.node];
    *col = node_col[t.node];
  };

  // the segments of an affine layer over the parts of an Append (for every time offset of a TdnnComponent); a part that is a Sum
  // is materialised first.  Returns the number of weight columns the parts cover.
  auto add_gemm_segs = [&](LayerOp *op, const std::vector<DescPart> &parts, int n, const std::vector<int> &toffs) {
    const NnetNode &nd = nodes[n];
    int wcol = 0;
    std::vector<int> sum_buf(parts.size(), -1);      // a materialised part's buffer: made once, read at every time offset
    for (int o2 : toffs) {
      for (auto &p : parts) {
        int sbuf, scol, soff;
        int &made = sum_buf[&p - &parts[0]];
        if (made >= 0) {
          sbuf = made; scol = 0; soff = 0;
        } else if (p.terms.size() == 1 && p.terms[0].scale == 1.0f) {
          const DescTerm &t = p.terms[0];
          term_src(t, &sbuf, &scol);
          soff = t.const_t ? 0 : t.offset;
          if (sbuf == -2) { sbuf = -1; soff = 0; }
          else if (t.const_t) Fail("nnet3: ReplaceIndex on a non-iVector node is not supported (node " + nd.name + ")");
        } else {
          // materialise the sum
          LayerOp sop;
          sop.kind = LayerOp::kEltwise;
          sop.name = nd.name + ".sum";
          sop.out_dim = p.dim;
          int l = 0, r = 0;
          for (int oo : toffs) { l = std::max(l, lext[n] - oo); r = std::max(r, rext[n] + oo); }
          sop.out_buf = new_buf(p.dim, std::max(l, 0), std::max(r, 0));
          for (auto &t : p.terms) {
            int b, c;
            term_src(t, &b, &c);
            if (b == -2 || t.const_t) Fail("nnet3: Sum() over the iVector input is not supported");
            sop.terms.push_back({b, c, t.offset, t.scale});
          }
          ops.push_back(sop);
          sbuf = made = sop.out_buf; scol = 0; soff = 0;
        }
        GemmSegment sg;
        sg.src_buf = sbuf; sg.src_col = scol; sg.ncols = p.dim; sg.offset = soff + (sbuf == -1 ? 0 : o2); sg.w_col = wcol;
        op->segs.push_back(sg);
        wcol += p.dim;
      }
    }
    return wcol;
  };

  for (int n : order) {
    NnetNode &nd = nodes[n];
    if (nd.kind == NnetNode::kInput) continue;
    if (block_of[n] >= 0) {
      // ---- a recurrent block: the feed-forward columns of W_all as a layer GEMM over all rows (bias included), then the walk
      const BlockNodes &b = blocks[block_of[n]];
      if (b.pgru) {
        // ---- a block around a GruNonlinearityComponent: the x-columns of W_z, W_r and W_hpart stacked to one layer GEMM of
        // cell + R + cell rows with their three biases (each element's sum over k is what its own affine would compute), then the walk
        const bool proj = b.wy >= 0;
        const int C = b.cell, R = b.rec_dim, l = lext[b.wa], r = rext[b.wa];
        const Component *aff[3] = {&components[nodes[b.wa].component], &components[nodes[b.wo].component], &components[nodes[b.hp].component]};
        const int aff_node[3] = {b.wa, b.wo, b.hp}, aff_rows[3] = {C, R, C}, aff_row0[3] = {0, C, C + R};
        // (the composed form, gru-layer / pgru-layer / norm-pgru-layer: the third affine is W_h.UW over Append(x, h1_t), its recurrent
        // columns are the cell x R matrix the walk multiplies with r . s; the block is named after y_t)
        const int in_dim = aff[2]->m.at("<LinearParams>").cols - (b.gruc ? R : 0), pre_dim = 2 * C + R;
        const int name_node = b.gruc ? b.sc : b.nl;
        LayerOp g;
        g.kind = LayerOp::kGemm;
        g.name = nodes[name_node].name + ".x";
        g.out_dim = pre_dim;
        g.W.Resize(pre_dim, in_dim);
        g.bias.assign(pre_dim, 0.0f);
        LayerOp w;
        w.kind = LayerOp::kPgru;
        w.name = nodes[name_node].name;
        w.out_dim = 2 * C;
        PgruBlock &k = w.pgru;
        k.W_zs.Resize(C, R);
        k.W_rs.Resize(R, R);
        for (int a = 0; a < 3; a++) {
          const MatF &W = aff[a]->m.at("<LinearParams>");
          for (int row = 0; row < aff_rows[a]; row++) {
            for (int c = 0; c < in_dim; c++) g.W(aff_row0[a] + row, c) = W(row, c);
            if (a == 0) for (int c = 0; c < R; c++) k.W_zs(row, c) = W(row, in_dim + c);
            if (a == 1) for (int c = 0; c < R; c++) k.W_rs(row, c) = W(row, in_dim + c);
          }
          auto bit = aff[a]->v.find("<BiasParams>");
          if (bit != aff[a]->v.end() && !bit->second.empty()) {
            if ((int)bit->second.size() != aff_rows[a]) Fail("nnet3: bias dim mismatch in node " + nodes[aff_node[a]].name);
            std::copy(bit->second.begin(), bit->second.end(), g.bias.begin() + aff_row0[a]);
          }
        }
        const int wcol = add_gemm_segs(&g, b.x_parts, b.wa, {0});
        if (wcol != in_dim) Fail("nnet3: internal error, the feed-forward input of recurrent block " + w.name + " does not cover its weights' columns");
        g.out_buf = new_buf(pre_dim, l, r);
        ops.push_back(g);
        k.in_dim = in_dim; k.cell = C;
        k.rec = proj ? R : 0;
        k.nonrec = proj ? nodes[b.wy].dim - R : 0;
        k.delay = b.delay;
        k.scale = TruncationScale(components[nodes[b.tr].component]);
        k.norm = b.nm >= 0;
        if (k.norm) { const Component &nc = components[nodes[b.nm].component]; k.target_rms = nc.f.count("<TargetRms>") ? (float)nc.f.at("<TargetRms>")[0] : 1.0f; }
        k.dropout = b.zd >= 0;
        k.composed = b.gruc;
        if (b.gruc) {
          const MatF &W = aff[2]->m.at("<LinearParams>");
          k.W_h.Resize(C, R);
          for (int row = 0; row < C; row++) for (int c = 0; c < R; c++) k.W_h(row, c) = W(row, in_dim + c);
        } else {
          // <w_h>: cell x R (the recogniser checked the shape; a one-row text matrix is in the vector map)
          const Component &nc = components[nodes[b.nl].component];
          auto mit = nc.m.find("<w_h>");
          if (mit != nc.m.end()) k.W_h = mit->second;
          else { k.W_h.Resize(1, R); const std::vector<float> &v = nc.v.at("<w_h>"); for (int c = 0; c < R; c++) k.W_h(0, c) = v[c]; }
        }
        if (proj) {
          const Component &wy = components[nodes[b.wy].component];
          k.W_y = wy.m.at("<LinearParams>");
          auto yb = wy.v.find("<BiasParams>");
          k.b_y = yb != wy.v.end() && !yb->second.empty() ? yb->second : std::vector<float>(k.W_y.rows, 0.0f);
          if ((int)k.b_y.size() != k.W_y.rows) Fail("nnet3: bias dim mismatch in node " + nodes[b.wy].name);
        }
        k.need_lext = b.need_lext;
        k.pre_buf = g.out_buf;
        k.hc_buf = new_buf(2 * C, l, r);
        if (proj) k.y_buf = new_buf(R + k.nonrec, l, r);
        k.s_buf = new_buf(R, l, r);
        if (!b.gruc) {
          node_buf[b.hp] = k.pre_buf;
          node_col[b.hp] = C + R;
          node_buf[b.nl] = k.hc_buf;
        }
        node_buf[b.sc] = k.hc_buf;
        node_col[b.sc] = C;
        if (proj) node_buf[b.wy] = node_buf[b.sp] = k.y_buf;
        node_buf[b.tr] = k.s_buf;
        w.out_buf = k.hc_buf;
        w.terms.push_back({k.pre_buf, 0, 0, 1.0f});
        ops.push_back(w);
        continue;
      }
      if (b.composed) {
        // ---- the composed LSTM(P) cell: the x-columns of W_i, W_f, W_c and W_o stacked to one layer GEMM of 4 cell rows with their
        // biases, in the gate order the kernel's weight image takes (each element's sum over k is what its own affine would compute),
        // their recurrent columns as W_r, the three peephole vectors as params, then the walk
        const int C = b.cell, R = b.rec_dim, l = lext[b.wa], r = rext[b.wa];
        const int in_dim = components[nodes[b.ga[0]].component].m.at("<LinearParams>").cols - R;
        LayerOp g;
        g.kind = LayerOp::kGemm;
        g.name = nodes[b.tr].name + ".x";
        g.out_dim = 4 * C;
        g.W.Resize(4 * C, in_dim);
        g.bias.assign(4 * C, 0.0f);
        LayerOp w;
        w.kind = LayerOp::kLstmp;
        w.name = nodes[b.tr].name;
        w.out_dim = 2 * C;
        LstmBlock &k = w.lstm;
        k.composed = true;
        k.W_r.Resize(4 * C, R);
        for (int a = 0; a < 4; a++) {
          const Component &ac = components[nodes[b.ga[a]].component];
          const MatF &W = ac.m.at("<LinearParams>");
          for (int row = 0; row < C; row++) {
            for (int c = 0; c < in_dim; c++) g.W(a * C + row, c) = W(row, c);
            for (int c = 0; c < R; c++) k.W_r(a * C + row, c) = W(row, in_dim + c);
          }
          auto bit = ac.v.find("<BiasParams>");
          if (bit != ac.v.end() && !bit->second.empty()) {
            if ((int)bit->second.size() != C) Fail("nnet3: bias dim mismatch in node " + nodes[b.ga[a]].name);
            std::copy(bit->second.begin(), bit->second.end(), g.bias.begin() + a * C);
          }
        }
        const int wcol = add_gemm_segs(&g, b.x_parts, b.wa, {0});
        if (wcol != in_dim) Fail("nnet3: internal error, the feed-forward input of recurrent block " + w.name + " does not cover its weights' columns");
        g.out_buf = new_buf(4 * C, l, r);
        ops.push_back(g);
        k.params.Resize(3, C);
        for (int p = 0; p < 3; p++) {
          const std::vector<float> &v = components[nodes[b.pe[p]].component].v.at("<Params>");
          for (int c = 0; c < C; c++) k.params(p, c) = v[c];
        }
        k.in_dim = in_dim; k.cell = C; k.rec = b.rp >= 0 ? R : 0; k.nonrec = b.rp >= 0 ? nodes[b.rp].dim - R : 0;
        k.delay = b.delay;
        k.scale = TruncationScale(components[nodes[b.tr].component]);        // (a ClipGradientComponent has no <Scale>: 1)
        k.scale_r = TruncationScale(components[nodes[b.sr].component]);
        k.dropout = b.cdrop;
        k.need_lext = b.need_lext;
        k.pre_buf = g.out_buf;
        k.cm_buf = new_buf(2 * C, l, r);           // [sc | m]
        k.st_buf = new_buf(C + R, l, r);           // [sc | sr]
        node_buf[b.m] = k.cm_buf;
        node_col[b.m] = C;
        node_buf[b.tr] = node_buf[b.sr] = k.st_buf;
        node_col[b.sr] = C;
        if (b.rp >= 0) {
          const Component &rp = components[nodes[b.rp].component];
          k.W_rp = rp.m.at("<LinearParams>");
          auto rb = rp.v.find("<BiasParams>");
          k.b_rp = rb != rp.v.end() && !rb->second.empty() ? rb->second : std::vector<float>(k.W_rp.rows, 0.0f);
          if ((int)k.b_rp.size() != k.W_rp.rows) Fail("nnet3: bias dim mismatch in node " + nodes[b.rp].name);
          k.rp_buf = new_buf(k.rec + k.nonrec, l, r);
          node_buf[b.rp] = node_buf[b.r] = k.rp_buf;
        }
        w.out_buf = k.cm_buf;
        w.terms.push_back({k.pre_buf, 0, 0, 1.0f});
        ops.push_back(w);
        continue;
      }
      if (b.gru) {
        // ---- a GRU block: the x-columns of W_z, W_o and W_hpart stacked to one layer GEMM of 3 cell rows with their biases (each
        // element's sum over k is what its own affine would compute), then the walk
        const int C = b.cell, R = b.rec_dim, l = lext[b.wa], r = rext[b.wa];
        const Component *aff[3] = {&components[nodes[b.wa].component], &components[nodes[b.wo].component], &components[nodes[b.hp].component]};
        const int in_dim = aff[2]->m.at("<LinearParams>").cols;
        const int name_node = b.gruc ? b.sc : b.nl;      // (the composed form, opgru-layer / norm-opgru-layer, is named after y_t)
        LayerOp g;
        g.kind = LayerOp::kGemm;
        g.name = nodes[name_node].name + ".x";
        g.out_dim = 3 * C;
        g.W.Resize(3 * C, in_dim);
        g.bias.assign(3 * C, 0.0f);
        LayerOp w;
        w.kind = LayerOp::kGru;
        w.name = nodes[name_node].name;
        w.out_dim = 2 * C;
        GruBlock &k = w.gru;
        k.W_s.Resize(2 * C, R);
        for (int a = 0; a < 3; a++) {
          const MatF &W = aff[a]->m.at("<LinearParams>");
          for (int row = 0; row < C; row++) {
            for (int c = 0; c < in_dim; c++) g.W(a * C + row, c) = W(row, c);
            if (a < 2) for (int c = 0; c < R; c++) k.W_s(a * C + row, c) = W(row, in_dim + c);
          }
          auto bit = aff[a]->v.find("<BiasParams>");
          if (bit != aff[a]->v.end() && !bit->second.empty()) {
            if ((int)bit->second.size() != C) Fail("nnet3: bias dim mismatch in node " + nodes[a == 0 ? b.wa : a == 1 ? b.wo : b.hp].name);
            std::copy(bit->second.begin(), bit->second.end(), g.bias.begin() + a * C);
          }
        }
        const int wcol = add_gemm_segs(&g, b.x_parts, b.wa, {0});
        if (wcol != in_dim) Fail("nnet3: internal error, the feed-forward input of recurrent block " + w.name + " does not cover its weights' columns");
        g.out_buf = new_buf(3 * C, l, r);
        ops.push_back(g);
        const Component &wy = components[nodes[b.wy].component];
        k.in_dim = in_dim; k.cell = C; k.rec = R; k.nonrec = nodes[b.wy].dim - R;
        k.delay = b.delay;
        k.scale = TruncationScale(components[nodes[b.tr].component]);
        k.norm = b.nm >= 0;
        if (k.norm) { const Component &nc = components[nodes[b.nm].component]; k.target_rms = nc.f.count("<TargetRms>") ? (float)nc.f.at("<TargetRms>")[0] : 1.0f; }
        k.dropout = b.zd >= 0;
        k.composed = b.gruc;
        k.w_h = b.gruc ? components[nodes[b.h2].component].v.at("<Params>") : components[nodes[b.nl].component].v.at("<w_h>");
        k.W_y = wy.m.at("<LinearParams>");
        auto yb = wy.v.find("<BiasParams>");
        k.b_y = yb != wy.v.end() && !yb->second.empty() ? yb->second : std::vector<float>(k.W_y.rows, 0.0f);
        if ((int)k.b_y.size() != k.W_y.rows) Fail("nnet3: bias dim mismatch in node " + nodes[b.wy].name);
        k.need_lext = b.need_lext;
        k.pre_buf = g.out_buf;
        k.hc_buf = new_buf(2 * C, l, r);
        k.y_buf = new_buf(R + k.nonrec, l, r);
        k.s_buf = new_buf(R, l, r);
        node_buf[b.hp] = k.pre_buf;
        node_col[b.hp] = 2 * C;
        if (!b.gruc) node_buf[b.nl] = k.hc_buf;
        node_buf[b.sc] = k.hc_buf;
        node_col[b.sc] = C;
        node_buf[b.wy] = node_buf[b.sp] = k.y_buf;
        node_buf[b.tr] = k.s_buf;
        w.out_buf = k.hc_buf;
        w.terms.push_back({k.pre_buf, 0, 0, 1.0f});
        ops.push_back(w);
        continue;
      }
      if (b.lstmb) {
        // ---- the cell behind a bottleneck: the x-columns of W_all_a as a layer GEMM of bottleneck rows (a LinearComponent: no
        // bias), its m-columns, W_all_b and the scale / offset vectors as the walk's operands
        const MatF &Wa = components[nodes[b.wa].component].m.at("<Params>"), &Wb = components[nodes[b.wb].component].m.at("<Params>");
        const int C = b.cell, B = Wa.rows, in_dim = Wa.cols - C, l = lext[b.wa], r = rext[b.wa];
        LayerOp g;
        g.kind = LayerOp::kGemm;
        g.name = nodes[b.wa].name + ".x";
        g.out_dim = B;
        g.W.Resize(B, in_dim);
        LayerOp w;
        w.kind = LayerOp::kLstmb;
        w.name = nodes[b.nl].name;
        w.out_dim = 2 * C;
        LstmBlock &k = w.lstm;
        k.W_r.Resize(B, C);
        for (int row = 0; row < B; row++) {
          for (int c = 0; c < in_dim; c++) g.W(row, c) = Wa(row, c);
          for (int c = 0; c < C; c++) k.W_r(row, c) = Wa(row, in_dim + c);
        }
        const int wcol = add_gemm_segs(&g, b.x_parts, b.wa, {0});
        if (wcol != in_dim) Fail("nnet3: internal error, the feed-forward input of recurrent block " + w.name + " does not cover its weights' columns");
        g.out_buf = new_buf(B, l, r);
        ops.push_back(g);
        k.W_b = Wb;
        ScaleAndOffsetVectors(components[nodes[b.so].component], component_names[nodes[b.so].component], &k.so_scale, &k.so_offset);
        k.in_dim = in_dim; k.cell = C; k.bottleneck = B;
        k.delay = b.delay;
        k.scale = TruncationScale(components[nodes[b.tr].component]);
        k.self_scale = b.self_scale;
        k.params = components[nodes[b.nl].component].m.at("<Params>");
        k.need_lext = b.need_lext;
        k.pre_buf = g.out_buf;
        k.cm_buf = new_buf(2 * C, l, r);           // [c | m]
        k.st_buf = new_buf(2 * C, l, r);           // [sc | sm]
        node_buf[b.nl] = k.cm_buf;
        node_buf[b.tr] = node_buf[b.sc] = node_buf[b.sr] = k.st_buf;
        node_col[b.sr] = C;
        w.out_buf = k.cm_buf;
        w.terms.push_back({k.pre_buf, 0, 0, 1.0f});
        ops.push_back(w);
        continue;
      }
      const Component &wa = components[nodes[b.wa].component];
      const MatF &W = wa.m.at("<LinearParams>");
      const int C = b.cell, rec = b.rec_dim, in_dim = W.cols - rec, l = lext[b.wa], r = rext[b.wa];
      LayerOp g;
      g.kind = LayerOp::kGemm;
      g.name = nodes[b.wa].name + ".x";
      g.out_dim = 4 * C;
      g.W.Resize(4 * C, in_dim);
      LayerOp w;
      w.kind = LayerOp::kLstm;
      w.name = nodes[b.nl].name;
      w.out_dim = 2 * C;
      LstmBlock &k = w.lstm;
      k.W_r.Resize(4 * C, rec);
      for (int row = 0; row < 4 * C; row++) {
        for (int c = 0; c < in_dim; c++) g.W(row, c) = W(row, c);
        for (int c = 0; c < rec; c++) k.W_r(row, c) = W(row, in_dim + c);
      }
      auto bit = wa.v.find("<BiasParams>");
      if (bit != wa.v.end() && !bit->second.empty()) {
        if ((int)bit->second.size() != 4 * C) Fail("nnet3: bias dim mismatch in node " + nodes[b.wa].name);
        g.bias = bit->second;
      }
      const int wcol = add_gemm_segs(&g, b.x_parts, b.wa, {0});
      if (wcol != in_dim)
        Fail("nnet3: component of node " + nodes[b.wa].name + " expects input dim " + std::to_string(W.cols) + " but its descriptor provides " +
             std::to_string(wcol + rec));
      g.out_buf = new_buf(4 * C, l, r);
      ops.push_back(g);
      k.in_dim = in_dim; k.cell = C; k.rec = b.rp >= 0 ? nodes[b.r].dim : 0; k.nonrec = b.rp >= 0 ? nodes[b.rp].dim - nodes[b.r].dim : 0;
      k.delay = b.delay;
      k.scale = TruncationScale(components[nodes[b.tr].component]);
      k.dropout_mask = b.dm >= 0;
      k.params = components[nodes[b.nl].component].m.at("<Params>");
      k.need_lext = b.need_lext;
      k.pre_buf = g.out_buf;
      k.cm_buf = new_buf(2 * C, l, r);
      k.st_buf = new_buf(C + rec, l, r);
      node_buf[b.wa] = k.pre_buf;
      node_buf[b.nl] = k.cm_buf;
      node_buf[b.tr] = node_buf[b.sc] = node_buf[b.sr] = k.st_buf;
      node_col[b.sr] = C;
      if (b.rp >= 0) {
        const Component &rp = components[nodes[b.rp].component];
        k.W_rp = rp.m.at("<LinearParams>");
        auto rb = rp.v.find("<BiasParams>");
        k.b_rp = rb != rp.v.end() && !rb->second.empty() ? rb->second : std::vector<float>(k.W_rp.rows, 0.0f);
        if ((int)k.b_rp.size() != k.W_rp.rows) Fail("nnet3: bias dim mismatch in node " + nodes[b.rp].name);
        k.rp_buf = new_buf(k.rec + k.nonrec, l, r);
        node_buf[b.c] = node_buf[b.m] = k.cm_buf;
        node_col[b.m] = C;
        node_buf[b.rp] = node_buf[b.r] = k.rp_buf;
      }
      w.out_buf = k.cm_buf;
      w.terms.push_back({k.pre_buf, 0, 0, 1.0f});
      ops.push_back(w);
      continue;
    }
    if (nd.kind == NnetNode::kDimRange) {
      if (node_buf[nd.range_node] == -2) Fail("nnet3: dim-range-node over the iVector input is not supported");
      node_buf[n] = node_buf[nd.range_node];
      node_col[n] = node_col[nd.range_node] + nd.range_offset;
      continue;
    }
    const Component *comp = nd.kind == NnetNode::kComponent ? &components[nd.component] : nullptr;
    bool affine = comp && IsAffineLike(comp->type);
    const bool conv = comp && comp->type == "TimeHeightConvolutionComponent", permute = comp && comp->type == "PermuteComponent";
    const bool attention = comp && comp->type == "RestrictedAttentionComponent";
    std::vector<EltStage> stages;
    bool elt = !affine && !conv && !permute && !attention && (comp == nullptr || EltStagesFor(*comp, nd.name, &stages));
    if (!affine && !elt && !conv && !permute && !attention)
      Fail("nnet3: component type " + comp->type + " (node " + nd.name + ") is not supported by the HIP acoustic-model kernels");

    // ---- fuse an elementwise node into its producer when it is the only consumer of a plain reference
    bool plain = nd.input.parts.size() == 1 && nd.input.parts[0].terms.size() == 1;
    if (elt && plain) {
      const DescTerm &t = nd.input.parts[0].terms[0];
      if (!t.const_t && t.offset == 0 && t.scale == 1.0f && consumers[t.node] == 1 && node_op[t.node] >= 0 &&
          node_col[t.node] == 0 && nodes[t.node].kind != NnetNode::kDimRange) {
        LayerOp &op = ops[node_op[t.node]];
        bool ok = true;
        // a row-wise reduction can only be fused when the op's tile covers the whole row; keep those standalone
        for (auto &s : stages) if (s.kind == EltStage::kLogSoftmax || s.kind == EltStage::kNormalize) ok = false;
        if (op.kind == LayerOp::kGather || op.kind == LayerOp::kAttention) ok = false;      // (a column gather and the attention kernel have no epilogue)
        // ... and nothing follows a row-wise stage inside its op (the row kernel applies that stage alone): relu or batchnorm behind a
        // NormalizeComponent, relu-renorm-layer's neighbour in the next layer, is an op of its own reading the normalised buffer
        // (a node without a stage -- NoOp, dropout, the output-node -- still joins it: a name for the same rows)
        for (auto &s : op.stages) if (!stages.empty() && (s.kind == EltStage::kLogSoftmax || s.kind == EltStage::kNormalize)) ok = false;
        if (ok) {
          op.stages.insert(op.stages.end(), stages.begin(), stages.end());
          op.name += "+" + nd.name;
          node_buf[n] = node_buf[t.node];
          node_col[n] = 0;
          node_op[n] = node_op[t.node];
          // the fused buffer must cover this node's extent as well (it does: same offsets), keep max
          bufs[node_buf[n]].lext = std::max(bufs[node_buf[n]].lext, lext[n]);
          bufs[node_buf[n]].rext = std::max(bufs[node_buf[n]].rext, rext[n]);
          continue;
        }
      }
    }

    LayerOp op;
    op.name = nd.name;
    op.out_dim = nd.dim;
    if (affine) {
      op.kind = LayerOp::kGemm;
      const MatF &W = comp->type == "LinearComponent" ? comp->m.at("<Params>") : comp->m.at("<LinearParams>");
      op.W = W;
      auto bit = comp->v.find("<BiasParams>");
      if (bit != comp->v.end() && !bit->second.empty()) op.bias = bit->second;
      std::vector<int> toffs = tdnn_offsets(nd);
      const int wcol = add_gemm_segs(&op, nd.input.parts, n, toffs);
      if (wcol != W.cols) Fail("nnet3: component of node " + nd.name + " expects input dim " + std::to_string(W.cols) + " but its descriptor provides " + std::to_string(wcol));
      if (!op.bias.empty() && (int)op.bias.size() != W.rows) Fail("nnet3: bias dim mismatch in node " + nd.name);
    } else if (conv) {
      op.kind = LayerOp::kConv;
      op.conv = ReadConvGeom(*comp, component_names[nd.component]);
      op.W = comp->m.at("<LinearParams>");
      op.bias = comp->v.at("<BiasParams>");
      if (nd.input.parts.size() != 1 || nd.input.parts[0].terms.size() != 1 || nd.input.parts[0].terms[0].scale != 1.0f)
        Fail("nnet3: the input of convolution node " + nd.name + " must be one node or an Offset() of one");
      const DescTerm &t = nd.input.parts[0].terms[0];
      int b, c;
      term_src(t, &b, &c);
      if (b == -2 || t.const_t) Fail("nnet3: a convolution over the iVector input is not supported (node " + nd.name + ")");
      if (nd.input.dim != op.conv.filters_in * op.conv.height_in)
        Fail("nnet3: convolution node " + nd.name + " expects input dim " + std::to_string(op.conv.filters_in * op.conv.height_in) +
             " but its descriptor provides " + std::to_string(nd.input.dim));
      for (int dt : op.conv.time_offsets) op.terms.push_back({b, c, t.offset + dt, 1.0f});
    } else if (attention) {
      // one term, the source: the rows of the C context positions follow from the op's geometry (AttentionGeom::TimeOffset)
      op.kind = LayerOp::kAttention;
      op.attention = ReadAttentionGeom(*comp, component_names[nd.component], nd.name);
      if (nd.input.parts.size() != 1 || nd.input.parts[0].terms.size() != 1 || nd.input.parts[0].terms[0].scale != 1.0f)
        Fail(AttentionInputRefusal(nd.name, false));
      const DescTerm &t = nd.input.parts[0].terms[0];
      int b, c;
      term_src(t, &b, &c);
      if (b == -2 || t.const_t) Fail(AttentionInputRefusal(nd.name, true));
      if (nd.input.dim != op.attention.InDim())
        Fail("nnet3: attention node " + nd.name + " expects input dim " + std::to_string(op.attention.InDim()) + " but its descriptor provides " +
             std::to_string(nd.input.dim));
      op.terms.push_back({b, c, t.offset, 1.0f});
    } else if (permute) {
      // out[:, i] = in[:, column_map[i]] (CopyCols, nnet-simple-component.cc:3990-3995) over the parts of an Append
      op.kind = LayerOp::kGather;
      const std::vector<int32_t> &cm = comp->iv.at("<ColumnMap>");
      if ((int)cm.size() != nd.input.dim)
        Fail("nnet3: PermuteComponent node " + nd.name + " has a column map of " + std::to_string(cm.size()) + " entries but its descriptor provides " +
             std::to_string(nd.input.dim));
      std::vector<int> part_col0;
      int col0 = 0;
      for (auto &p : nd.input.parts) {
        if (p.terms.size() != 1 || p.terms[0].scale != 1.0f) Fail("nnet3: a Sum() or Scale() feeding PermuteComponent node " + nd.name + " is not supported");
        int b, c;
        term_src(p.terms[0], &b, &c);
        if (b == -2 || p.terms[0].const_t) Fail("nnet3: PermuteComponent node " + nd.name + " reads the iVector input directly: not supported");
        op.terms.push_back({b, c, p.terms[0].offset, 1.0f});
        part_col0.push_back(col0);
        col0 += p.dim;
      }
      std::vector<char> seen(cm.size(), 0);
      for (int32_t src : cm) {
        if (src < 0 || src >= (int)cm.size() || seen[src]) Fail("nnet3: PermuteComponent node " + nd.name + ": Column map does not represent a permutation.");
        seen[src] = 1;
        int part = (int)(std::upper_bound(part_col0.begin(), part_col0.end(), (int)src) - part_col0.begin()) - 1;
        op.gather_part.push_back(part);
        op.gather_col.push_back(src - part_col0[part]);
      }
    } else {
      op.kind = LayerOp::kEltwise;
      if (nd.input.parts.size() != 1) {
        // Append feeding an elementwise component / the output: copy each part into its column range
        Fail("nnet3: Append() feeding a non-affine component (node " + nd.name + ") is not supported");
      }
      for (auto &t : nd.input.parts[0].terms) {
        int b, c;
        term_src(t, &b, &c);
        if (b == -2 || t.const_t) Fail("nnet3: elementwise component over the iVector input is not supported (node " + nd.name + ")");
        op.terms.push_back({b, c, t.offset, t.scale});
      }
      op.stages = stages;
      bool row_wise = false;
      for (auto &s : stages) if (s.kind == EltStage::kLogSoftmax || s.kind == EltStage::kNormalize) row_wise = true;
      if (row_wise && (op.terms.size() != 1 || op.terms[0].scale != 1.0f)) {
        // the row kernel reads one unscaled source: a Sum() or Scale() in front of it is materialised first, as add_gemm_segs does
        LayerOp sop;
        sop.kind = LayerOp::kEltwise;
        sop.name = nd.name + ".sum";
        sop.out_dim = nd.dim;
        sop.terms = op.terms;
        sop.out_buf = new_buf(nd.dim, lext[n], rext[n]);
        ops.push_back(sop);
        op.terms.assign(1, SumTerm{sop.out_buf, 0, 0, 1.0f});
      }
      if (nd.kind == NnetNode::kOutput && op.terms.size() == 1 && op.terms[0].offset == 0 && op.terms[0].scale == 1.0f &&
          op.terms[0].src_col == 0 && bufs[op.terms[0].src_buf].dim == nd.dim && op.stages.empty()) {
        // output-node that simply names a buffer: alias it
        node_buf[n] = op.terms[0].src_buf;
        node_op[n] = -1;
        continue;
      }
    }
    op.out_buf = new_buf(nd.dim, lext[n], rext[n]);
    ops.push_back(op);
    node_buf[n] = op.out_buf;
    node_col[n] = 0;
    node_op[n] = (int)ops.size() - 1;
  }
  output_buf = node_buf[out_node];
  if (output_buf < 0 || node_col[out_node] != 0 || bufs[output_buf].dim != output_dim)
    Fail("nnet3: could not resolve the output node to a buffer");
  // ---- a two-term sum whose one term is the (otherwise unread) result of a GEMM becomes that GEMM's epilogue: the residual of a
  // factorised TDNN layer, NoOp(Sum(Scale(0.66, previous layer), dropout(batchnorm(relu(affine))))) -- as a separate pass over two
  // 1024-wide buffers it took as long as the layer's two GEMMs together (profiles/r06/tdnnf_notes.txt).  RS_FUSE_RESIDUAL=0 keeps
  // the elementwise op (tests compare the two bit for bit).
  {
    const char *e = std::getenv("RS_FUSE_RESIDUAL");
    const bool fuse = !(e && std::atoi(e) == 0);
    auto readers = [&](int buf) {
      int n = buf == output_buf ? 1 : 0;
      for (auto &op : ops) {
        for (auto &sg : op.segs) n += sg.src_buf == buf;
        for (auto &t : op.terms) n += t.src_buf == buf;
        n += op.res_buf == buf;
      }
      return n;
    };
    for (size_t ei = 0; fuse && ei < ops.size(); ei++) {
      LayerOp &eo = ops[ei];
      if (eo.kind != LayerOp::kEltwise || eo.terms.size() != 2 || !eo.stages.empty()) continue;
      for (int k = 0; k < 2; k++) {
        const SumTerm &t = eo.terms[k], &r = eo.terms[1 - k];
        if (t.scale != 1.0f || t.offset != 0 || r.offset != 0 || t.src_col != 0 || r.src_col != 0 || t.src_buf == r.src_buf) continue;
        if (bufs[t.src_buf].dim != eo.out_dim || bufs[r.src_buf].dim != eo.out_dim || readers(t.src_buf) != 1) continue;
        size_t gi = ops.size(), ri = 0;
        bool r_made = bufs[r.src_buf].is_input;
        for (size_t i = 0; i < ei; i++) {
          if (ops[i].out_buf == t.src_buf) gi = i;
          if (ops[i].out_buf == r.src_buf) { ri = i; r_made = true; }
        }
        if (gi == ops.size() || ops[gi].kind != LayerOp::kGemm || ops[gi].res_buf >= 0 || !r_made || (ri >= gi && !bufs[r.src_buf].is_input)) continue;
        for (auto &st : ops[gi].stages) if (st.kind == EltStage::kLogSoftmax || st.kind == EltStage::kNormalize) gi = ops.size();
        if (gi == ops.size()) continue;
        LayerOp &g = ops[gi];
        g.res_buf = r.src_buf;
        g.res_scale = r.scale;
        g.out_buf = eo.out_buf;
        g.name += "+" + eo.name;
        ops.erase(ops.begin() + ei);
        ei--;
        break;
      }
    }
  }
  // sanity: every source buffer must cover what its consumers read
  for (auto &op : ops) {
    const BufferInfo &ob = bufs[op.out_buf];
    auto check = [&](int sb, int off) {
      if (sb < 0) return;
      if (bufs[sb].lext < ob.lext - off || bufs[sb].rext < ob.rext + off)
        Fail("nnet3: internal error, buffer extents of op " + op.name + " are inconsistent");
    };
    for (auto &s : op.segs) check(s.src_buf, s.offset);
    for (auto &t : op.terms) {
      check(t.src_buf, t.offset);
      if (op.kind == LayerOp::kAttention)
        for (int o = 0; o < op.attention.Context(); o++) check(t.src_buf, t.offset + op.attention.TimeOffset(o));
    }
    check(op.res_buf, 0);
  }
}

// --frame-subsampling-factor f: the output is wanted at t = 0, f, 2 f, ... only (CreateComputationRequestInternal, nnet-compile-looped.cc:
// 111-128) and the reference's compiler computes of every layer just the rows something reads.  Same here, in the one form a TDNN
// stack needs: walking the ops backwards, the residues (t mod f) of every buffer that are read; a buffer read at residue 0 only is
// evaluated on every f-th row (chain models: everything above the last layer with offsets that are not multiples of f).
void Nnet::SetSubsampling(int factor) {
  for (auto &b : bufs) b.stride = 1;
  if (factor <= 1 || factor > 30 || output_buf < 0) return;
  std::vector<unsigned> need(bufs.size(), 0u);
  need[output_buf] = 1u;
  auto mod = [&](int a) { int r = a % factor; return r < 0 ? r + factor : r; };
  // (elementwise ops -- a TDNN-F layer's Sum(Scale(0.66, x), y), a row-wise component -- take row lists like the GEMMs (RunNnet), so
  // they propagate the residues they are read at like any other op.  Round 5 forced their buffers dense AFTER the walk, which left
  // a layer X that feeds a Sum dense while its own input W stayed strided: X's GEMM ran over all rows and read rows of W nobody
  // had written in that call.)
  for (auto it = ops.rbegin(); it != ops.rend(); ++it) {
    if (it->kind == LayerOp::kLstm || it->kind == LayerOp::kLstmp || it->kind == LayerOp::kLstmb) {
      // a block's buffers hold the same rows: every residue one of them is read at, and every residue the chains of those rows
      // pass through (delay 3 under factor 3 stays in its class; delay 2 visits all three)
      const LstmBlock &k = it->lstm;
      unsigned all = need[k.cm_buf] | need[k.st_buf] | (k.rp_buf >= 0 ? need[k.rp_buf] : 0u);
      for (int round = 0; round < factor; round++)
        for (int r = 0; r < factor; r++) if (all >> r & 1u) all |= 1u << mod(r - k.delay);
      need[k.cm_buf] = need[k.st_buf] = all;
      if (k.rp_buf >= 0) need[k.rp_buf] = all;
    }
    if (it->kind == LayerOp::kGru) {      // (the same rule for a GRU block's three buffers)
      const GruBlock &k = it->gru;
      unsigned all = need[k.hc_buf] | need[k.y_buf] | need[k.s_buf];
      for (int round = 0; round < factor; round++)
        for (int r = 0; r < factor; r++) if (all >> r & 1u) all |= 1u << mod(r - k.delay);
      need[k.hc_buf] = need[k.y_buf] = need[k.s_buf] = all;
    }
    if (it->kind == LayerOp::kPgru) {      // (... and for a block around a GruNonlinearityComponent; no y buffer without a projection)
      const PgruBlock &k = it->pgru;
      unsigned all = need[k.hc_buf] | need[k.s_buf] | (k.y_buf >= 0 ? need[k.y_buf] : 0u);
      for (int round = 0; round < factor; round++)
        for (int r = 0; r < factor; r++) if (all >> r & 1u) all |= 1u << mod(r - k.delay);
      need[k.hc_buf] = need[k.s_buf] = all;
      if (k.y_buf >= 0) need[k.y_buf] = all;
    }
    const unsigned out = need[it->out_buf];
    auto reads = [&](int src, int off) {
      if (src < 0) return;
      for (int r = 0; r < factor; r++) if (out >> r & 1u) need[src] |= 1u << mod(r + off);
    };
    for (auto &sg : it->segs) reads(sg.src_buf, sg.offset);
    for (auto &t : it->terms) {
      if (it->kind == LayerOp::kAttention)      // (the rows of its context positions)
        for (int o = 0; o < it->attention.Context(); o++) reads(t.src_buf, t.offset + it->attention.TimeOffset(o));
      else
        reads(t.src_buf, t.offset);
    }
    reads(it->res_buf, 0);
  }
  for (size_t b = 0; b < bufs.size(); b++) if (!bufs[b].is_input && need[b] == 1u) bufs[b].stride = factor;
}

void AcousticModel::Read(const std::string &final_mdl, int frames_per_chunk, int extra_left_context_initial, int frame_subsampling_factor) {
  KaldiReader r(final_mdl);
  trans.Read(r);
  nnet.Read(r, frames_per_chunk, extra_left_context_initial, frame_subsampling_factor);
  r.ExpectToken("<LeftContext>");
  r.ReadInt32();
  r.ExpectToken("<RightContext>");
  r.ReadInt32();
  r.ExpectToken("<Priors>");
  r.ReadVector(&nnet.priors);
  if (!nnet.priors.empty() && (int)nnet.priors.size() != nnet.output_dim) nnet.priors.clear();  // am-nnet-simple.cc:63-68
  if (trans.num_pdfs != nnet.output_dim)
    Fail(final_mdl + ": transition model has " + std::to_string(trans.num_pdfs) + " pdfs but the nnet output dim is " + std::to_string(nnet.output_dim));
  nnet.Compile();
  nnet.SetSubsampling(frame_subsampling_factor);
}

// =============================================================================== HCLG

namespace {
struct ByteReader {
  const std::string &b;
  size_t p = 0;
  const std::string &name;
  ByteReader(const std::string &bytes, const std::string &n) : b(bytes), name(n) {}
  template <typename T> T Get() {
    if (p + sizeof(T) > b.size()) Fail(name + ": truncated FST file");
    T v;
    std::memcpy(&v, b.data() + p, sizeof(T));
    p += sizeof(T);
    return v;
  }
  std::string Str() {
    int32_t n = Get<int32_t>();
    if (n < 0 || p + (size_t)n > b.size()) Fail(name + ": bad string in FST header");
    std::string s = b.substr(p, n);
    p += n;
    return s;
  }
  void SkipSymbolTable() {
    // openfst lib/symbol-table.cc SymbolTableImpl::Read: magic, name, available_key, size, then (symbol, key)*
    int32_t magic = Get<int32_t>();
    if (magic != 2125658996) Fail(name + ": bad symbol table magic");
    Str();
    Get<int64_t>();
    int64_t n = Get<int64_t>();
    for (int64_t i = 0; i < n; i++) { Str(); Get<int64_t>(); }
  }
};
}  // namespace

void Hclg::Read(const std::string &path) {
  std::string bytes = ReadFileBytes(path);
  ByteReader r(bytes, path);
  if (r.Get<int32_t>() != 2125659606) Fail("FstHeader::Read: Bad FST header: " + path);
  std::string fsttype = r.Str(), arctype = r.Str();
  int32_t version = r.Get<int32_t>(), flags = r.Get<int32_t>();
  r.Get<uint64_t>();  // properties
  int64_t st = r.Get<int64_t>(), ns = r.Get<int64_t>(), na = r.Get<int64_t>();
  if (arctype != "standard") Fail("FST with arc type " + arctype + " not supported.");   // kaldi-fst-io.cc:66-69
  if (flags & 1) r.SkipSymbolTable();
  if (flags & 2) r.SkipSymbolTable();
  if (ns <= 0 || st < 0 || st >= ns) Fail(path + ": empty FST or no start state");
  start = (int32_t)st;
  auto align = [&]() { while (r.p % 16) r.p++; };   // MappedFile::kArchAlignment
  if (fsttype == "const") {
    bool aligned = (version == 1) || (flags & 4);
    if (aligned) align();
    final_cost.resize(ns);
    arc_begin.resize(ns + 1);
    num_ieps.resize(ns);
    for (int64_t s = 0; s < ns; s++) {
      final_cost[s] = r.Get<float>();
      uint32_t pos = r.Get<uint32_t>(), narcs = r.Get<uint32_t>(), nie = r.Get<uint32_t>();
      r.Get<uint32_t>();
      arc_begin[s] = pos;
      num_ieps[s] = nie;
      if (s + 1 == ns) arc_begin[ns] = pos + narcs;
      else if (false) (void)narcs;
    }
    if (aligned) align();
    if (arc_begin[ns] != (uint64_t)na) Fail(path + ": ConstFst arc count mismatch");
    arcs.resize(na);
    if (r.p + (size_t)na * sizeof(FstArc) > bytes.size()) Fail(path + ": truncated ConstFst arcs");
    std::memcpy(arcs.data(), bytes.data() + r.p, (size_t)na * sizeof(FstArc));
    for (int64_t s = 0; s + 1 < ns; s++) if (arc_begin[s] > arc_begin[s + 1]) Fail(path + ": ConstFst states are not in arc order");
  } else if (fsttype == "vector") {
    final_cost.resize(ns);
    arc_begin.resize(ns + 1);
    num_ieps.assign(ns, 0);
    arcs.clear();
    for (int64_t s = 0; s < ns; s++) {
      final_cost[s] = r.Get<float>();
      int64_t n = r.Get<int64_t>();
      arc_begin[s] = (uint32_t)arcs.size();
      for (int64_t a = 0; a < n; a++) {
        FstArc arc;
        arc.ilabel = r.Get<int32_t>();
        arc.olabel = r.Get<int32_t>();
        arc.weight = r.Get<float>();
        arc.nextstate = r.Get<int32_t>();
        if (arc.ilabel == 0) num_ieps[s]++;
        arcs.push_back(arc);
      }
    }
    arc_begin[ns] = (uint32_t)arcs.size();
  } else {
    Fail("Reading FST: unsupported FST type: " + fsttype);   // kaldi-fst-io.cc:86-89
  }
  for (auto &a : arcs)
    if (a.nextstate < 0 || a.nextstate >= ns || a.ilabel < 0) Fail(path + ": arc with invalid next state or label");
}

std::vector<std::string> ReadWordsTxt(const std::string &path) {
  std::ifstream is(path);
  if (!is.good()) Fail("Could not read symbol table from file " + path);
  std::vector<std::string> out;
  std::string sym;
  long id;
  while (is >> sym >> id) {
    if (id < 0) continue;
    if ((long)out.size() <= id) out.resize(id + 1);
    out[id] = sym;
  }
  return out;
}

}  // namespace rs
