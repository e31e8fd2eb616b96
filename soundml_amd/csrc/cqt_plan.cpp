// Cqt.Config.create (cqt.ml:121-424) on the host, in float64: the frequency ladder, the relative bandwidths, the fractional
// filter lengths and the main-lobe cutoff, the early decimations, the octave plan and one filter bank per octave, with the
// reference's validation and messages.  The octave kernel of cqt.ml:202-247 is built as the reference builds it (periodic
// window over floor(l/2) - floor(-l/2) points, unit `norm`-norm, l / n_fft rescale, centre pad, forward transform, the
// non-redundant half kept) and then stored in the form the device consumes: its time-domain taps
//   g[b, n] = sum_{k <= n_fft / 2} K[b, k] exp(-2 pi i k n / n_fft)
// (the transform of the half spectrum extended by zeros), for which K . rfft(frame) = sum_n frame[n] g[b, n].
// The 0/1 chroma fold of chroma.ml:332-366 lives here too.
#include <cfloat>
#include <complex>

#include "smx_internal.hpp"

namespace smx {
namespace {

using cplx = std::complex<double>;

// in-place forward transform of n = 2^k points: bit reversal, then radix-2 passes against exp(-2 pi i j / n) evaluated entry by entry
void fft_pow2(std::vector<cplx> &a, const std::vector<cplx> &roots) {
  const size_t n = a.size();
  for (size_t i = 1, j = 0; i < n; ++i) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  for (size_t len = 2; len <= n; len <<= 1) {
    const size_t step = n / len;
    for (size_t i = 0; i < n; i += len)
      for (size_t j = 0; j < len / 2; ++j) {
        const cplx u = a[i + j], v = a[i + j + len / 2] * roots[j * step];
        a[i + j] = u + v;
        a[i + j + len / 2] = u - v;
      }
  }
}

// cqt.ml:31-54: the equivalent noise bandwidth of the window in FFT bins; the table, else measured on 1000 periodic points
double window_enbw(int kind, double param) {
  switch (kind) {
    case SMX_WINDOW_HANN: return 1.50018310546875;
    case SMX_WINDOW_HAMMING: return 1.3629455320350348;
    case SMX_WINDOW_BLACKMAN: return 1.7269681554262326;
    case SMX_WINDOW_BLACKMAN_HARRIS: return 2.0045975283585014;
    case SMX_WINDOW_NUTTALL: return 1.9763500280946082;
    case SMX_WINDOW_BARTLETT: return 1.3334961334912805;
    case SMX_WINDOW_FLAT_TOP: return 2.7762255046484143;
    case SMX_WINDOW_RECTANGULAR: return 1.0;
    default: break;
  }
  std::vector<double> w(1000);
  window_make_param(kind, param, true, 1000, w.data());
  double sum = 0.0, squares = 0.0;
  for (double v : w) {
    sum += v;
    squares += v * v;
  }
  return 1000.0 * squares / (sum * sum);
}

// Window.make reports domain errors under its own entry point; relabel them with this one (cqt.ml:273-285)
template <typename F>
auto relabel_window(F &&f) -> decltype(f()) {
  try {
    return f();
  } catch (const InvalidArgument &e) {
    const std::string m = e.what();
    const size_t colon = m.find(':');
    throw InvalidArgument(colon == std::string::npos ? "create: " + m : "create" + m.substr(colon));
  }
}

void check_positive_int(const char *name, int64_t value, int64_t floor) {   // cqt.ml:261-265
  if (value < floor)
    throw InvalidArgument(format("create: cannot use %s = %lld (%s must be at least %lld)", name, (long long)value, name, (long long)floor));
}

void check_finite(const char *name, double value, bool ok, const char *description) {   // cqt.ml:267-271
  if (!(std::isfinite(value) && ok))
    throw InvalidArgument(format("create: cannot use %s = %g (%s must be %s)", name, value, name, description));
}

// Float.pow 2. e through libm's pow, as the reference evaluates it: the compiler would otherwise turn a literal base 2 into exp2,
// which differs from pow in the last place on some arguments
double pow_two(double e) {
  volatile double two = 2.0;
  return std::pow(two, e);
}

int64_t two_factors(int64_t x) {   // cqt.ml:61-63
  int64_t n = 0;
  while (x > 0 && x % 2 == 0) {
    ++n;
    x /= 2;
  }
  return n;
}

// cqt.ml:174-177: Q_k sr / (f_k + gamma_k / alpha_k), Q_k = filter_scale / alpha_k, for bins [first, first + count)
std::vector<double> filter_lengths_at(const smx_cqt_config &c, int64_t first, int64_t count, double sample_rate) {
  std::vector<double> out((size_t)count);
  for (int64_t j = 0; j < count; ++j) {
    const size_t k = (size_t)(first + j);
    const double q = c.filter_scale / c.alphas[k];
    out[(size_t)j] = q * sample_rate / (c.freqs[k] + (c.gammas[k] / c.alphas[k]));
  }
  return out;
}

// cqt.ml:202-247, then the time-domain form; `gain` is sqrt(base_rate / rate) (cqt.ml:373-374)
std::vector<double> octave_taps(const smx_cqt_config &c, int64_t first, const std::vector<double> &lengths, double sample_rate,
                                int64_t n_fft, double gain) {
  const int64_t m = (int64_t)lengths.size();
  const bool unit_norm = c.norm == 1.0;
  std::vector<cplx> roots((size_t)std::max<int64_t>(1, n_fft / 2));
  for (size_t j = 0; j < roots.size(); ++j) {
    const double a = -2.0 * M_PI * (double)j / (double)n_fft;
    roots[j] = cplx(std::cos(a), std::sin(a));
  }
  std::vector<double> taps((size_t)(m * n_fft * 2));
  std::vector<cplx> line((size_t)n_fft);
  std::vector<double> coefficients;
  for (int64_t j = 0; j < m; ++j) {
    const double length = lengths[(size_t)j], freq = c.freqs[(size_t)(first + j)];
    const int64_t lo = (int64_t)std::floor(-length / 2.0), hi = (int64_t)std::floor(length / 2.0);
    const int64_t count = hi - lo;
    coefficients.assign((size_t)count, 0.0);
    window_make_param(c.window, c.window_param, true, count, coefficients.data());
    std::fill(line.begin(), line.end(), cplx(0.0, 0.0));
    const int64_t left = (n_fft - count) / 2;
    double mass = 0.0;
    for (int64_t i = 0; i < count; ++i) {
      const double t = (double)(lo + i);
      const double angle = t * 2.0 * M_PI * freq / sample_rate;
      const double a = std::cos(angle) * coefficients[(size_t)i], b = std::sin(angle) * coefficients[(size_t)i];
      line[(size_t)(left + i)] = cplx(a, b);
      const double modulus = std::hypot(a, b);
      mass += unit_norm ? modulus : std::pow(modulus, c.norm);
    }
    if (!unit_norm) mass = std::pow(mass, 1.0 / c.norm);
    if (mass < DBL_MIN) mass = 1.0;   // an all-but-vanishing filter is left unnormalised (cqt.ml:230-233)
    const double rescale = length / (double)n_fft;
    for (int64_t i = 0; i < count; ++i) {
      cplx &v = line[(size_t)(left + i)];
      v = cplx(v.real() / mass * rescale, v.imag() / mass * rescale);
    }
    fft_pow2(line, roots);
    for (int64_t k = 0; k < n_fft; ++k) line[(size_t)k] = k <= n_fft / 2 ? line[(size_t)k] * gain : cplx(0.0, 0.0);
    fft_pow2(line, roots);
    for (int64_t n = 0; n < n_fft; ++n) {
      taps[(size_t)((j * n_fft + n) * 2)] = line[(size_t)n].real();
      taps[(size_t)((j * n_fft + n) * 2 + 1)] = line[(size_t)n].imag();
    }
  }
  return taps;
}

double round_half_even(double x) {   // chroma.ml:87-93
  const double below = std::floor(x), fraction = x - below;
  if (fraction > 0.5) return below + 1.0;
  if (fraction < 0.5) return below;
  return std::fmod(below, 2.0) == 0.0 ? below : below + 1.0;
}

}  // namespace

smx_cqt_config *cqt_config_create(int64_t n_bins, int64_t sample_rate, double fmin, int64_t bins_per_octave, int gamma, double gamma_value,
                                  double tuning, double filter_scale, double norm, int window, double window_param, bool scale,
                                  int64_t hop, int pad, double pad_value) {
  check_positive_int("n_bins", n_bins, 1);
  check_positive_int("bins_per_octave", bins_per_octave, 1);
  check_positive_int("hop", hop, 1);
  check_positive_int("sample_rate", sample_rate, 1);
  check_finite("fmin", fmin, fmin > 0.0, "finite and positive");
  check_finite("tuning", tuning, true, "finite");
  check_finite("filter_scale", filter_scale, filter_scale > 0.0, "finite and positive");
  check_finite("norm", norm, norm > 0.0, "finite and positive");
  if (gamma < SMX_CQT_GAMMA_CONSTANT_Q || gamma > SMX_CQT_GAMMA_FIXED) throw Failure(format("create: unknown gamma mode %d", gamma));
  if (gamma == SMX_CQT_GAMMA_FIXED) check_finite("gamma", gamma_value, gamma_value >= 0.0, "finite and non-negative");
  if (pad < SMX_PAD_REFLECT || pad > SMX_PAD_EDGE) throw Failure(format("create: unknown pad mode %d", pad));
  if (window == SMX_WINDOW_CUSTOM) throw Failure("create: the filter envelope is a window family, not a table");
  const double enbw = relabel_window([&] { return window_enbw(window, window_param); });

  auto c = std::make_unique<smx_cqt_config>();
  c->fmin = fmin; c->bins_per_octave = bins_per_octave; c->gamma = gamma; c->gamma_value = gamma_value; c->tuning = tuning;
  c->filter_scale = filter_scale; c->norm = norm; c->window = window; c->window_param = window_param; c->scale = scale;
  c->hop = hop; c->pad = pad; c->pad_value = pad_value; c->n_bins = n_bins; c->sample_rate = sample_rate;

  // the ladder, octave by octave: a bin and its octave transposition differ by exactly a factor of two (cqt.ml:121-131)
  const double anchor = fmin * pow_two(tuning / (double)bins_per_octave);
  std::vector<double> ratios((size_t)bins_per_octave);
  for (int64_t j = 0; j < bins_per_octave; ++j) ratios[(size_t)j] = pow_two((double)j / (double)bins_per_octave);
  c->freqs.resize((size_t)n_bins);
  bool finite = true;
  for (int64_t k = 0; k < n_bins; ++k) {
    const double f = pow_two((double)(k / bins_per_octave)) * ratios[(size_t)(k % bins_per_octave)] * anchor;
    c->freqs[(size_t)k] = f;
    finite = finite && std::isfinite(f);
  }
  if (!finite)
    throw InvalidArgument(format("create: cannot place %lld bins from %g Hz at %lld bins per octave (the frequency ladder overflows)",
                                 (long long)n_bins, fmin, (long long)bins_per_octave));
  // relative bandwidths from the numerical log2 difference, so that they carry the ladder's own rounding (cqt.ml:140-159)
  c->alphas.resize((size_t)n_bins);
  if (n_bins == 1) {
    const double r = pow_two(1.0 / (double)bins_per_octave);
    c->alphas[0] = ((r * r) - 1.0) / ((r * r) + 1.0);
  } else {
    std::vector<double> logf((size_t)n_bins);
    for (int64_t k = 0; k < n_bins; ++k) logf[(size_t)k] = std::log2(c->freqs[(size_t)k]);
    for (int64_t k = 0; k < n_bins; ++k) {
      const double b = k == 0 ? 1.0 / (logf[1] - logf[0])
                     : k == n_bins - 1 ? 1.0 / (logf[(size_t)(n_bins - 1)] - logf[(size_t)(n_bins - 2)])
                                       : 2.0 / (logf[(size_t)(k + 1)] - logf[(size_t)(k - 1)]);
      const double r = pow_two(2.0 / b);
      c->alphas[(size_t)k] = (r - 1.0) / (r + 1.0);
    }
  }
  c->gammas.resize((size_t)n_bins);   // cqt.ml:161-168
  for (int64_t k = 0; k < n_bins; ++k)
    c->gammas[(size_t)k] = gamma == SMX_CQT_GAMMA_CONSTANT_Q ? 0.0 : gamma == SMX_CQT_GAMMA_FIXED ? gamma_value : c->alphas[(size_t)k] * 24.7 / 0.108;
  const double sr = (double)sample_rate;
  c->lengths = filter_lengths_at(*c, 0, n_bins, sr);
  double cutoff = -INFINITY;   // cqt.ml:183-193
  int64_t limit = 0;
  for (int64_t k = 0; k < n_bins; ++k) {
    const double q = filter_scale / c->alphas[(size_t)k];
    const double v = (c->freqs[(size_t)k] * (1.0 + (0.5 * enbw / q))) + (0.5 * c->gammas[(size_t)k]);
    if (v > cutoff) {
      cutoff = v;
      limit = k;
    }
  }
  c->cutoff = cutoff;
  const double nyquist = sr / 2.0;
  if (cutoff > nyquist)
    throw InvalidArgument(format("create: cannot place %lld bins from %g Hz at a sample rate of %lld Hz (bin %lld, centred at %g Hz, "
                                 "reaches %g Hz, above the Nyquist frequency %g)", (long long)n_bins, fmin, (long long)sample_rate,
                                 (long long)limit, c->freqs[(size_t)limit], cutoff, nyquist));
  c->n_octaves = (n_bins + bins_per_octave - 1) / bins_per_octave;
  const int64_t n_filters = std::min(bins_per_octave, n_bins);
  // early decimation drops the rate to just above what the filters need, while the hop keeps a factor of two for every
  // remaining octave (cqt.ml:336-345)
  const int64_t head = std::max<int64_t>(0, (int64_t)std::ceil(std::log2(nyquist / cutoff)) - 2);
  const int64_t tail = std::max<int64_t>(0, two_factors(hop) - c->n_octaves + 1);
  c->early = std::min(head, tail);
  const double base_rate = sr / (double)(int64_t(1) << c->early);
  double rate = base_rate;
  int64_t octave_hop = hop / (int64_t(1) << c->early), halved = 0;
  for (int64_t i = 0; i < c->n_octaves; ++i) {
    smx_cqt_config::Octave o;
    o.first = std::max<int64_t>(0, n_bins - (n_filters * (i + 1)));
    o.count = n_bins - (n_filters * i) - o.first;
    const std::vector<double> lengths = filter_lengths_at(*c, o.first, o.count, rate);
    double longest = 0.0;
    for (double l : lengths) longest = std::max(longest, l);
    const double exponent = std::ceil(std::log2(longest));   // cqt.ml:67-69 next_power_of_two
    o.n_fft = exponent >= 0.0 && exponent < 40.0 ? int64_t(1) << (int)exponent : (exponent < 0.0 ? 0 : -1);
    if (o.n_fft < 1)
      throw InvalidArgument(format("create: cannot resolve %lld bins from %g Hz with filter_scale = %g (the filters of octave %lld span "
                                   "less than one sample)", (long long)n_bins, fmin, filter_scale, (long long)i));
    o.hop = octave_hop;
    o.halvings = halved;
    // every octave analyses the same band of the decimated signal, so its response carries the energy of the whole rate
    // reduction it sits under (cqt.ml:370-374)
    o.taps = relabel_window([&] { return octave_taps(*c, o.first, lengths, rate, o.n_fft, std::sqrt(base_rate / rate)); });
    c->octaves.push_back(std::move(o));
    if (octave_hop % 2 == 0) {
      octave_hop /= 2;
      rate /= 2.0;
      ++halved;
    }
  }
  c->divisors.assign((size_t)n_bins, 1.0);   // cqt.ml:389-402
  if (scale) {
    const std::vector<double> at_base = filter_lengths_at(*c, 0, n_bins, base_rate);
    for (int64_t k = 0; k < n_bins; ++k) c->divisors[(size_t)k] = std::sqrt(at_base[(size_t)k]);
  }
  if (smx_resample_config_create(2, 1, SMX_RESAMPLE_HIGH, 0.0, 0.0, &c->half) != SMX_OK) throw Failure(smx_last_error());   // cqt.ml:417
  return c.release();
}

std::vector<double> cqt_fold_matrix(const char *op, const smx_cqt_config &c, int64_t n_chroma) {
  if (n_chroma < 1)   // chroma.ml:347-358
    throw InvalidArgument(format("%s: cannot build %lld chroma bands (n_chroma must be at least 1)", op, (long long)n_chroma));
  if (c.bins_per_octave % n_chroma != 0)
    throw InvalidArgument(format("%s: cannot fold %lld bins per octave onto %lld chroma bands (bins_per_octave must be an integer "
                                 "multiple of n_chroma)", op, (long long)c.bins_per_octave, (long long)n_chroma));
  const int64_t merge = c.bins_per_octave / n_chroma;
  // MIDI numbers count twelve semitones to the octave whatever the chroma resolution (chroma.ml:332-345)
  double midi = (12.0 * (std::log2(c.fmin) - std::log2(440.0))) + 69.0;
  midi = std::fmod(std::fmod(midi, 12.0) + 12.0, 12.0);
  const int64_t shift = (int64_t)round_half_even(midi * ((double)n_chroma / 12.0));
  std::vector<double> w((size_t)(n_chroma * c.n_bins), 0.0);
  for (int64_t ch = 0; ch < n_chroma; ++ch) {
    const int64_t source = (((ch - shift) % n_chroma) + n_chroma) % n_chroma;
    for (int64_t k = 0; k < c.n_bins; ++k) {
      const int64_t step = ((k % c.bins_per_octave) + (merge / 2)) % c.bins_per_octave;
      if (step / merge == source) w[(size_t)(ch * c.n_bins + k)] = 1.0;
    }
  }
  return w;
}

}  // namespace smx

int64_t smx_cqt_config::frames(int64_t n) const {   // cqt.ml:543-556; Stft.frames of the centered analysis (stft.ml:217-223)
  if (n < 0)
    throw smx::InvalidArgument(smx::format("frames: cannot analyse a signal of length %lld (length must be non-negative)", (long long)n));
  int64_t least = INT64_MAX;
  for (const Octave &o : octaves) {
    const int64_t d = int64_t(1) << (early + o.halvings);
    const int64_t len = (n + d - 1) / d, padded = len + 2 * (o.n_fft / 2);
    const int64_t count = len == 0 || padded < o.n_fft ? 0 : 1 + (padded - o.n_fft) / o.hop;
    least = std::min(least, count);
  }
  return least;
}

int64_t smx_cqt_config::latency() const {   // cqt.ml:471-479: max over octaves of D (L - 1) + K (D - 1) + 1
  const int64_t k = smx_resample_config_latency(half);
  int64_t worst = 0;
  for (const Octave &o : octaves) {
    const int64_t d = int64_t(1) << (early + o.halvings);
    worst = std::max(worst, d * (o.n_fft / 2 - 1) + k * (d - 1) + 1);
  }
  return worst;
}

// ---- the streaming schedule (Cqt.Kernel, cqt.ml:694-1012): host integers only, cqt_stream.hip runs by them -----------------------
namespace smx {

namespace {
// resample.ml:1298 `ready` of the 2:1 plan: the outputs whose every input is among the first `fed` samples
int64_t halved_ready(int64_t fed, int64_t lag) { return fed > lag ? (fed - lag + 1) / 2 : 0; }
int64_t ceil_div_pos(int64_t a, int64_t b) { return a <= 0 ? 0 : (a + b - 1) / b; }
}  // namespace

// frames of octave `o` whose every sample is among the first `seen` of its stream: frame p ends at p hop + n_fft - n_fft / 2.
// Under Reflect frame 0 also reads sample n_fft / 2 (the mirror of its first), so nothing is ready before seen > n_fft / 2
// (the install threshold left_width + 1 of stft.ml:447-452).
int64_t cqt_octave_ready(const smx_cqt_config &c, const smx_cqt_config::Octave &o, int64_t seen) {
  const int64_t reach = o.n_fft - o.n_fft / 2;
  if (seen < reach || (c.pad == SMX_PAD_REFLECT && seen < o.n_fft / 2 + 1)) return 0;
  return (seen - reach) / o.hop + 1;
}

// columns every octave has produced once `fed` samples went in: the chain of 2:1 stages, then the slowest octave
int64_t cqt_columns_ready(const smx_cqt_config &c, int64_t fed) {
  const int64_t lag = smx_resample_config_latency(c.half);
  int64_t least = INT64_MAX, level = 0, seen = fed;
  for (const smx_cqt_config::Octave &o : c.octaves) {   // levels only grow down the plan
    for (; level < c.early + o.halvings; ++level) seen = halved_ready(seen, lag);
    least = std::min(least, cqt_octave_ready(c, o, seen));
  }
  return least;
}

// the most columns an octave holds that the slowest has not reached: octave i trails the input by less than the plan's
// latency less D_i n_fft_i / 2 samples of it, and a column is `hop` of them
int64_t cqt_run_ahead(const smx_cqt_config &c) {
  const int64_t latency = c.latency();
  int64_t worst = 0;
  for (const smx_cqt_config::Octave &o : c.octaves) {
    const int64_t d = int64_t(1) << (c.early + o.halvings);
    worst = std::max(worst, ceil_div_pos(latency - d * (o.n_fft / 2), c.hop) + 1);
  }
  return worst;
}

// the most columns one step of at most max_block samples, or the flush, returns: a step moves the gate by its samples over the
// hop, rounded up, and once more where the gate opens; the flush returns what the latency withheld
int64_t cqt_column_bound(const smx_cqt_config &c, int64_t max_block) {
  return std::max(ceil_div_pos(max_block, c.hop) + 1, ceil_div_pos(c.latency(), c.hop) + 1);
}

}  // namespace smx
