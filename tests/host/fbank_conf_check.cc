// Host-only check of the filterbank configuration (rhasspy_speech_amd/csrc/model.{h,cc}): ReadFbankOptions + BuildFbankTables over
// the fbank.conf files named on the command line, built by tests/test_fbank_cpu.py under the address and undefined-behaviour
// sanitizers.  Arguments: pairs of <case name> <path of fbank.conf, or - for no file: the defaults>.  Per case one line
//   <name> dim=<row width> bins=<mel bins> energy_col=<column or -1> mel_col0=<first mel column> padded=<FFT points> weights=<n>
// after the tables have been walked the way the kernel walks them (every filter inside the power spectrum, every weight in [0, 1],
// every column the kernel writes inside the row); `<name> error: <message>` when the reader or the builder refuses the file.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>

#include "../../rhasspy_speech_amd/csrc/model.h"

static void Require(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "fbank_conf_check: %s\n", what); std::exit(2); }
}

int main(int argc, char **argv) {
  Require(argc >= 3 && argc % 2 == 1, "usage: fbank_conf_check <name> <fbank.conf | -> ...");
  for (int a = 1; a + 1 < argc; a += 2) {
    const std::string name = argv[a], path = argv[a + 1];
    try {
      rs::FbankOptions o;
      if (path != "-") rs::ReadFbankOptions(path, &o);
      rs::MfccTables t;
      rs::BuildFbankTables(o, &t);
      Require(t.fbank && t.nbins == o.num_bins && t.nceps == o.Dim() && t.nceps <= 128, "row width");
      Require((int)t.window.size() == t.win && t.win <= t.padded, "window");
      Require((int)t.mel_offset.size() == t.nbins && (int)t.mel_len.size() == t.nbins && (int)t.mel_start.size() == t.nbins, "filter tables");
      size_t weights = 0;
      for (int b = 0; b < t.nbins; b++) {
        // the kernel reads power-spectrum bins [offset, offset + len) of padded / 2 + 1 and weights [start, start + len)
        Require(t.mel_offset[b] >= 0 && t.mel_len[b] >= 1 && t.mel_offset[b] + t.mel_len[b] <= t.padded / 2, "filter outside the spectrum");
        Require(t.mel_start[b] == (int)weights && weights + t.mel_len[b] <= t.mel_weights.size(), "filter outside the weights");
        for (int i = 0; i < t.mel_len[b]; i++) {
          const float w = t.mel_weights[weights + i];
          Require(w >= 0.0f && w <= 1.0f, "weight outside [0, 1]");
        }
        weights += t.mel_len[b];
      }
      Require(weights == t.mel_weights.size(), "weights left over");
      // columns: mel bin b -> mel_col0 + b, the energy -> energy_col; together exactly [0, dim)
      Require(t.mel_col0 + t.nbins <= t.nceps && t.energy_col < t.nceps, "column outside the row");
      Require(t.opts.use_energy ? (t.energy_col == (t.mel_col0 == 1 ? 0 : t.nbins)) : (t.energy_col == -1 && t.mel_col0 == 0), "energy column");
      std::printf("%s dim=%d bins=%d energy_col=%d mel_col0=%d padded=%d weights=%zu\n", name.c_str(), t.nceps, t.nbins, t.energy_col, t.mel_col0,
                  t.padded, weights);
    } catch (const std::exception &e) {
      std::printf("%s error: %s\n", name.c_str(), e.what());
    }
  }
  return 0;
}
