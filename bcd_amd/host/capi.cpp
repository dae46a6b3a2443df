// capi.cpp -- plain-C exports of libbcdcore for the Python plumbing (bench.py, tests): synthetic scenes,
// the SamplesAccumulator, Utils packing, and the bcd::Denoiser / bcd::MultiscaleDenoiser classes themselves.
#include "Denoiser.h"
#include "DeviceSamplesAccumulator.h"
#include "MultiscaleDenoiser.h"
#include "SamplesAccumulator.h"
#include "SequenceDenoiser.h"
#include "SpikeRemovalFilter.h"
#include "SyntheticScene.h"
#include "Utils.h"

#include <algorithm>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

using namespace bcd;

extern "C" {

// W x i_nbOfLines band of a W x H synthetic frame; outputs: ns [n], mean [n*3], cov [n*6], hist [n*60]
int bcdcore_synthetic_scene_ex(int W, int H, int spp, unsigned seed, float sigma, float spikeProbability, int pattern, int firstLine, int nbOfLines,
		float* o_ns, float* o_mean, float* o_cov, float* o_hist);

int bcdcore_synthetic_scene(int W, int H, int spp, unsigned seed, float sigma, float spikeProbability, int firstLine, int nbOfLines,
		float* o_ns, float* o_mean, float* o_cov, float* o_hist)
{
	return bcdcore_synthetic_scene_ex(W, H, spp, seed, sigma, spikeProbability, 0, firstLine, nbOfLines, o_ns, o_mean, o_cov, o_hist);
}

int bcdcore_synthetic_scene_ex(int W, int H, int spp, unsigned seed, float sigma, float spikeProbability, int pattern, int firstLine, int nbOfLines,
		float* o_ns, float* o_mean, float* o_cov, float* o_hist)
{
	if(W <= 0 || H <= 0 || spp <= 0 || firstLine < 0 || firstLine + nbOfLines > H) return -1;
	SyntheticSceneParameters p;
	p.m_width = W; p.m_height = H; p.m_samplesPerPixel = spp; p.m_seed = seed; p.m_noiseSigma = sigma; p.m_spikeProbability = spikeProbability;
	p.m_pattern = pattern;
	SamplesStatisticsImages st = generateSyntheticScene(p, firstLine, nbOfLines);
	st.m_nbOfSamplesImage.copyDataTo(o_ns);
	st.m_meanImage.copyDataTo(o_mean);
	st.m_covarImage.copyDataTo(o_cov);
	st.m_histoImage.copyDataTo(o_hist);
	return 0;
}

// samples: n x (line, col, r, g, b, weight)
int bcdcore_accumulate(const float* s, long long n, int W, int H, int nbins, float gamma, float maxval, float* ns, float* mean, float* cov, float* hist)
{
	HistogramParameters hp;
	hp.m_nbOfBins = nbins; hp.m_gamma = gamma; hp.m_maxValue = maxval;
	SamplesAccumulator acc(W, H, hp);
	for(long long i = 0; i < n; ++i, s += 6)
		acc.addSample(int(s[0]), int(s[1]), s[2], s[3], s[4], s[5]);
	SamplesStatisticsImages st = acc.getSamplesStatistics();
	st.m_nbOfSamplesImage.copyDataTo(ns);
	st.m_meanImage.copyDataTo(mean);
	st.m_covarImage.copyDataTo(cov);
	st.m_histoImage.copyDataTo(hist);
	return 0;
}

// the same through SamplesAccumulatorThreadSafe::addSampleThreadSafely from `threads` OpenMP threads that share the sample list
// round-robin (so that threads do meet on the same pixel)
int bcdcore_accumulate_threadsafe(const float* s, long long n, int W, int H, int nbins, float gamma, float maxval, int threads, float* ns, float* mean,
		float* cov, float* hist)
{
	HistogramParameters hp;
	hp.m_nbOfBins = nbins; hp.m_gamma = gamma; hp.m_maxValue = maxval;
	SamplesAccumulatorThreadSafe acc(W, H, hp);
#pragma omp parallel for schedule(static, 1) num_threads(threads)
	for(long long i = 0; i < n; ++i)
	{
		const float* p = s + 6 * i;
		acc.addSampleThreadSafely(int(p[0]), int(p[1]), p[2], p[3], p[4], p[5]);
	}
	SamplesStatisticsImages st = acc.getSamplesStatistics();
	st.m_nbOfSamplesImage.copyDataTo(ns);
	st.m_meanImage.copyDataTo(mean);
	st.m_covarImage.copyDataTo(cov);
	st.m_histoImage.copyDataTo(hist);
	return 0;
}

// the same stream through bcd::DeviceSamplesAccumulator::addSample on `device`; a non-destructive host snapshot is taken after the first
// `snapshot_at` samples (0: none) and the accumulation goes on.  Returns 0, or -1 with the class's message in bcdcore_device_accumulate_error()
static std::string g_deviceAccumulateError;
const char* bcdcore_device_accumulate_error() { return g_deviceAccumulateError.c_str(); }

int bcdcore_device_accumulate(const float* s, long long n, int W, int H, int nbins, float gamma, float maxval, int device, long long snapshot_at,
		float* ns, float* mean, float* cov, float* hist)
{
	HistogramParameters hp;
	hp.m_nbOfBins = nbins; hp.m_gamma = gamma; hp.m_maxValue = maxval;
	DeviceSamplesAccumulator acc(W, H, hp, device);
	g_deviceAccumulateError.clear();
	if(!acc.isValid()) { g_deviceAccumulateError = acc.lastError(); return -1; }
	for(long long i = 0; i < n; ++i, s += 6)
	{
		if(i == snapshot_at && snapshot_at > 0)
			(void)acc.getSamplesStatistics();
		acc.addSample(int(s[0]), int(s[1]), s[2], s[3], s[4], s[5]);
	}
	SamplesStatisticsImages st = acc.extractSamplesStatistics();
	if(!acc.lastError().empty()) { g_deviceAccumulateError = acc.lastError(); return -1; }
	st.m_nbOfSamplesImage.copyDataTo(ns);
	st.m_meanImage.copyDataTo(mean);
	st.m_covarImage.copyDataTo(cov);
	st.m_histoImage.copyDataTo(hist);
	return 0;
}

// a stream of mixed calls through bcd::DeviceSamplesAccumulator: n x (kind, a, b, r, g, b, weight); kind 0: addSample(line = a, col = b),
// kind 1: splatSample(x = a, y = b), with the filter (radii, table[tableSize^2]) set first.  counts[2]: samples accumulated / dropped
int bcdcore_device_splat(const float* s, long long n, int W, int H, int nbins, float gamma, float maxval, int device, float radiusX, float radiusY,
		int tableSize, const float* table, float* ns, float* mean, float* cov, float* hist, long long* counts)
{
	HistogramParameters hp;
	hp.m_nbOfBins = nbins; hp.m_gamma = gamma; hp.m_maxValue = maxval;
	DeviceSamplesAccumulator acc(W, H, hp, device);
	g_deviceAccumulateError.clear();
	if(!acc.isValid()) { g_deviceAccumulateError = acc.lastError(); return -1; }
	if(!acc.setFilter(radiusX, radiusY, tableSize, table)) { g_deviceAccumulateError = acc.lastError(); return -1; }
	for(long long i = 0; i < n; ++i, s += 7)
	{
		if(s[0] != 0.f) acc.splatSample(s[1], s[2], s[3], s[4], s[5], s[6]);
		else acc.addSample(int(s[1]), int(s[2]), s[3], s[4], s[5], s[6]);
	}
	counts[0] = acc.nbOfAccumulatedSamples();
	counts[1] = acc.nbOfDroppedSamples();
	SamplesStatisticsImages st = acc.extractSamplesStatistics();
	if(!acc.lastError().empty()) { g_deviceAccumulateError = acc.lastError(); return -1; }
	st.m_nbOfSamplesImage.copyDataTo(ns);
	st.m_meanImage.copyDataTo(mean);
	st.m_covarImage.copyDataTo(cov);
	st.m_histoImage.copyDataTo(hist);
	return 0;
}

// mixed calls through the batch forms of a bcd::DeviceSamplesAccumulator with `nbLayers` colour layers: s is n x (kind, a, b, r, g, b, weight)
// as for bcdcore_device_splat, layerRgb [nbLayers][n][3] the layers' colours of the same calls.  Runs of one kind go through addSamples /
// splatSamples in pieces of at most `batch` calls; a host snapshot of the beauty and of one layer is taken before call `snapshotAt` (0: none).
// statePath / layersPath (both or neither): the state and the layer block are saved at the end and loaded into a second accumulator, whose
// statistics are the ones returned.  lmean [nbLayers][H][W][3], lcov [nbLayers][H][W][6]; counts[2]: samples accumulated / dropped
int bcdcore_device_accumulate_layers(const float* s, long long n, const float* layerRgb, int nbLayers, int W, int H, int nbins, float gamma,
		float maxval, int device, float radiusX, float radiusY, int tableSize, const float* table, long long batch, long long snapshotAt,
		const char* statePath, const char* layersPath, float* ns, float* mean, float* cov, float* hist, float* lmean, float* lcov, long long* counts)
{
	HistogramParameters hp;
	hp.m_nbOfBins = nbins; hp.m_gamma = gamma; hp.m_maxValue = maxval;
	g_deviceAccumulateError.clear();
	DeviceSamplesAccumulator first(W, H, hp, nbLayers, device);
	if(!first.isValid() || first.nbOfLayers() != nbLayers) { g_deviceAccumulateError = first.lastError(); return -1; }
	if(table && !first.setFilter(radiusX, radiusY, tableSize, table)) { g_deviceAccumulateError = first.lastError(); return -1; }
	std::vector<int32_t> pixels;
	std::vector<float> keys, rgb, weights;
	std::vector<std::vector<float>> layers((size_t)nbLayers);
	std::vector<const float*> layerPointers((size_t)nbLayers);
	if(batch < 1) batch = n > 0 ? n : 1;
	for(long long i = 0; i < n; )
	{
		const bool splat = s[7 * i] != 0.f;
		long long e = i + 1;
		while(e < n && e - i < batch && (s[7 * e] != 0.f) == splat && !(snapshotAt > 0 && e == snapshotAt)) ++e;
		if(snapshotAt > 0 && i == snapshotAt)
		{
			Deepimf m, c;
			(void)first.getSamplesStatistics();
			if(!first.getLayerStatistics(nbLayers - 1, m, c)) { g_deviceAccumulateError = first.lastError(); return -1; }
		}
		const size_t m = size_t(e - i);
		pixels.resize(m); keys.resize(2 * m); rgb.resize(3 * m); weights.resize(m);
		for(size_t j = 0; j < m; ++j)
		{
			const float* p = s + 7 * (i + (long long)j);
			const int line = int(p[1]), col = int(p[2]);
			pixels[j] = (line < 0 || line >= H || col < 0 || col >= W) ? -1 : line * W + col;
			keys[2 * j] = p[1]; keys[2 * j + 1] = p[2];
			rgb[3 * j] = p[3]; rgb[3 * j + 1] = p[4]; rgb[3 * j + 2] = p[5];
			weights[j] = p[6];
		}
		for(int l = 0; l < nbLayers; ++l)
			layerPointers[(size_t)l] = layerRgb + 3 * ((long long)l * n + i);
		if(splat) first.splatSamples(keys.data(), rgb.data(), layerPointers.data(), weights.data(), (int64_t)m);
		else first.addSamples(pixels.data(), rgb.data(), layerPointers.data(), weights.data(), (int64_t)m);
		i = e;
	}
	std::unique_ptr<DeviceSamplesAccumulator> second;
	DeviceSamplesAccumulator* acc = &first;
	if(statePath && layersPath)
	{
		if(!first.saveState(statePath) || !first.saveLayers(layersPath)) { g_deviceAccumulateError = first.lastError(); return -1; }
		second.reset(new DeviceSamplesAccumulator(W, H, hp, nbLayers, device));
		if(!second->isValid() || !second->loadState(statePath) || !second->loadLayers(layersPath)) { g_deviceAccumulateError = second->lastError(); return -1; }
		acc = second.get();
	}
	counts[0] = acc->nbOfAccumulatedSamples();
	counts[1] = acc->nbOfDroppedSamples();
	for(int l = 0; l < nbLayers; ++l)
	{
		Deepimf m, c;
		if(!acc->getLayerStatistics(l, m, c)) { g_deviceAccumulateError = acc->lastError(); return -1; }
		m.copyDataTo(lmean + (size_t)l * W * H * 3);
		c.copyDataTo(lcov + (size_t)l * W * H * 6);
	}
	// the forms without layers are refused on this accumulator, each with a message and without touching the sums
	const float one[3] = { 1.f, 1.f, 1.f };
	const int32_t zero = 0;
	acc->addSample(0, 0, 1.f, 1.f, 1.f);
	const bool refusedSingle = acc->lastError().find("addSample") != std::string::npos;
	acc->addSamples(&zero, one, nullptr, 1);
	const bool refusedBatch = acc->lastError().find("addSamples") != std::string::npos;
	if(!refusedSingle || !refusedBatch || acc->nbOfAccumulatedSamples() != counts[0])
	{
		g_deviceAccumulateError = "an add without layers was accepted by an accumulator with layers";
		return -1;
	}
	SamplesStatisticsImages st = acc->getSamplesStatistics();
	st.m_nbOfSamplesImage.copyDataTo(ns);
	st.m_meanImage.copyDataTo(mean);
	st.m_covarImage.copyDataTo(cov);
	st.m_histoImage.copyDataTo(hist);
	return 0;
}

// mixed calls through the batch forms of a bcd::DeviceSamplesAccumulator with `nbFeatures` feature channels and `nbLayers` (0: none) colour
// layers: s, layerRgb, batch and the filter as for bcdcore_device_accumulate_layers, features [n][nbFeatures] the feature channels of the same
// calls.  statePath / layersPath / featuresPath (all or none; layersPath is not used without layers): the blocks are saved at the end and
// loaded into a second accumulator, whose statistics are the ones returned; mergeAgain: the same files are then merged into it once more
// (every running sum doubles).  fmean, fvar [H][W][nbFeatures]; lmean, lcov as there; counts[2]: samples accumulated / dropped
int bcdcore_device_accumulate_features(const float* s, long long n, const float* layerRgb, int nbLayers, const float* features, int nbFeatures, int W,
		int H, int nbins, float gamma, float maxval, int device, float radiusX, float radiusY, int tableSize, const float* table, long long batch,
		const char* statePath, const char* layersPath, const char* featuresPath, int mergeAgain, float* ns, float* mean, float* cov, float* hist,
		float* lmean, float* lcov, float* fmean, float* fvar, long long* counts)
{
	HistogramParameters hp;
	hp.m_nbOfBins = nbins; hp.m_gamma = gamma; hp.m_maxValue = maxval;
	g_deviceAccumulateError.clear();
	DeviceSamplesAccumulator first(W, H, hp, nbLayers, nbFeatures, device);
	if(!first.isValid() || first.nbOfLayers() != nbLayers || first.nbOfFeatures() != nbFeatures) { g_deviceAccumulateError = first.lastError(); return -1; }
	if(table && !first.setFilter(radiusX, radiusY, tableSize, table)) { g_deviceAccumulateError = first.lastError(); return -1; }
	std::vector<int32_t> pixels;
	std::vector<float> keys, rgb, weights;
	std::vector<const float*> layerPointers((size_t)nbLayers);
	if(batch < 1) batch = n > 0 ? n : 1;
	for(long long i = 0; i < n; )
	{
		const bool splat = s[7 * i] != 0.f;
		long long e = i + 1;
		while(e < n && e - i < batch && (s[7 * e] != 0.f) == splat) ++e;
		const size_t m = size_t(e - i);
		pixels.resize(m); keys.resize(2 * m); rgb.resize(3 * m); weights.resize(m);
		for(size_t j = 0; j < m; ++j)
		{
			const float* p = s + 7 * (i + (long long)j);
			const int line = int(p[1]), col = int(p[2]);
			pixels[j] = (line < 0 || line >= H || col < 0 || col >= W) ? -1 : line * W + col;
			keys[2 * j] = p[1]; keys[2 * j + 1] = p[2];
			rgb[3 * j] = p[3]; rgb[3 * j + 1] = p[4]; rgb[3 * j + 2] = p[5];
			weights[j] = p[6];
		}
		for(int l = 0; l < nbLayers; ++l)
			layerPointers[(size_t)l] = layerRgb + 3 * ((long long)l * n + i);
		const float* const* layers = nbLayers > 0 ? layerPointers.data() : nullptr;
		if(splat) first.splatSamples(keys.data(), rgb.data(), layers, features + (long long)nbFeatures * i, weights.data(), (int64_t)m);
		else first.addSamples(pixels.data(), rgb.data(), layers, features + (long long)nbFeatures * i, weights.data(), (int64_t)m);
		i = e;
	}
	std::unique_ptr<DeviceSamplesAccumulator> second;
	DeviceSamplesAccumulator* acc = &first;
	if(statePath && featuresPath)
	{
		if(!first.saveState(statePath) || !first.saveFeatures(featuresPath) || (nbLayers > 0 && !first.saveLayers(layersPath)))
		{
			g_deviceAccumulateError = first.lastError();
			return -1;
		}
		second.reset(new DeviceSamplesAccumulator(W, H, hp, nbLayers, nbFeatures, device));
		if(!second->isValid() || !second->loadState(statePath) || !second->loadFeatures(featuresPath) || (nbLayers > 0 && !second->loadLayers(layersPath))
				|| (mergeAgain && (!second->mergeState(statePath) || !second->mergeFeatures(featuresPath) || (nbLayers > 0 && !second->mergeLayers(layersPath)))))
		{
			g_deviceAccumulateError = second->lastError();
			return -1;
		}
		acc = second.get();
	}
	counts[0] = acc->nbOfAccumulatedSamples();
	counts[1] = acc->nbOfDroppedSamples();
	for(int l = 0; l < nbLayers; ++l)
	{
		Deepimf m, c;
		if(!acc->getLayerStatistics(l, m, c)) { g_deviceAccumulateError = acc->lastError(); return -1; }
		m.copyDataTo(lmean + (size_t)l * W * H * 3);
		c.copyDataTo(lcov + (size_t)l * W * H * 6);
	}
	Deepimf fm, fv;
	if(!acc->getFeatureStatistics(fm, fv)) { g_deviceAccumulateError = acc->lastError(); return -1; }
	const DeviceSamplesAccumulator::DeviceFeatureStatistics d = acc->computeDeviceFeatureStatistics();
	if(!d.m_pFeatures || !d.m_pVariances || d.m_nbOfChannels != nbFeatures) { g_deviceAccumulateError = acc->lastError(); return -1; }
	fm.copyDataTo(fmean);
	fv.copyDataTo(fvar);
	SamplesStatisticsImages st = acc->getSamplesStatistics();
	if(!acc->lastError().empty()) { g_deviceAccumulateError = acc->lastError(); return -1; }
	st.m_nbOfSamplesImage.copyDataTo(ns);
	st.m_meanImage.copyDataTo(mean);
	st.m_covarImage.copyDataTo(cov);
	st.m_histoImage.copyDataTo(hist);
	return 0;
}

// the refusals of a bcd::DeviceSamplesAccumulator(8 x 8, nbLayers, nbFeatures) that need no device: `messages` receives, one per line,
// lastError() after the constructor, after addSample, splatSample, the batch addSamples without features, addSamples with null features and
// splatSamples with null features.  Returns isValid() after the constructor
int bcdcore_device_features_refusals(int nbLayers, int nbFeatures, int device, char* messages, int capacity)
{
	HistogramParameters hp;
	DeviceSamplesAccumulator acc(8, 8, hp, nbLayers, nbFeatures, device);
	const int valid = acc.isValid() ? 1 : 0;
	std::string out = acc.lastError() + "\n";
	const float one[3] = { 1.f, 1.f, 1.f }, xy[2] = { 1.f, 1.f };
	const std::vector<const float*> layerColours(16, one);
	const float* const* layers = layerColours.data();
	const int32_t zero = 0;
	acc.addSample(0, 0, 1.f, 1.f, 1.f);
	out += acc.lastError() + "\n";
	acc.splatSample(1.f, 1.f, 1.f, 1.f, 1.f);
	out += acc.lastError() + "\n";
	acc.addSamples(&zero, one, nullptr, 1);
	out += acc.lastError() + "\n";
	acc.addSamples(&zero, one, nbLayers > 0 ? layers : nullptr, nullptr, nullptr, 1);
	out += acc.lastError() + "\n";
	acc.splatSamples(xy, one, nbLayers > 0 ? layers : nullptr, nullptr, nullptr, 1);
	out += acc.lastError() + "\n";
	if(valid && acc.nbOfAccumulatedSamples() != 0) out += "a refused add was applied\n";
	std::snprintf(messages, size_t(capacity), "%s", out.c_str());
	return valid;
}

// the same stream through bcd::DeviceSamplesAccumulator::addSample (no explicit flush), then one planSamples; pixels[budget] receives the
// list, summary[4] planned / active / unsampled / max_error.  invalidFirst: two invalid planSamples come first (a budget of 2^31 while the
// samples are still buffered, then max_per_pixel 0), and each must return false with a message.  Returns the number of planned samples,
// -1 (message as above) or -2 (an invalid call was accepted)
long long bcdcore_device_plan(const float* s, long long n, int W, int H, int nbins, float gamma, float maxval, int device, long long budget,
		unsigned long long offset, float threshold, float eps, float minSamples, int maxPerPixel, int invalidFirst, int* pixels, double* summary)
{
	HistogramParameters hp;
	hp.m_nbOfBins = nbins; hp.m_gamma = gamma; hp.m_maxValue = maxval;
	DeviceSamplesAccumulator acc(W, H, hp, device);
	g_deviceAccumulateError.clear();
	if(!acc.isValid()) { g_deviceAccumulateError = acc.lastError(); return -1; }
	for(long long i = 0; i < n; ++i, s += 6)
		acc.addSample(int(s[0]), int(s[1]), s[2], s[3], s[4], s[5]);
	DeviceSamplesAccumulator::PlanParameters prm;
	prm.m_threshold = threshold; prm.m_eps = eps; prm.m_minSamples = minSamples; prm.m_maxPerPixel = maxPerPixel;
	DeviceSamplesAccumulator::PlanSummary sum;
	std::vector<int32_t> list;
	if(invalidFirst)
	{
		DeviceSamplesAccumulator::PlanParameters bad = prm;
		bad.m_maxPerPixel = 0;
		if(acc.planSamples((long long)1 << 31, offset, prm, list, &sum) || acc.lastError().empty())
			return -2;
		if(acc.planSamples(budget, offset, bad, list, &sum) || acc.lastError().empty())
			return -2;
	}
	if(!acc.planSamples(budget, offset, prm, list, &sum)) { g_deviceAccumulateError = acc.lastError(); return -1; }
	std::copy(list.begin(), list.end(), pixels);
	summary[0] = double(sum.m_planned); summary[1] = double(sum.m_active); summary[2] = double(sum.m_unsampled); summary[3] = sum.m_maxError;
	return (long long)list.size();
}

// a bcd::DeviceSamplesAccumulator kept between calls, so that tests drive its state methods (exportState, saveState, loadState, mergeState,
// merge).  Every int call returns 0, or -1 with the class's message in bcdcore_device_acc_error(handle)
void* bcdcore_device_acc_create(int W, int H, int nbins, float gamma, float maxval, int device)
{
	HistogramParameters hp;
	hp.m_nbOfBins = nbins; hp.m_gamma = gamma; hp.m_maxValue = maxval;
	return new DeviceSamplesAccumulator(W, H, hp, device);
}

void bcdcore_device_acc_destroy(void* h) { delete (DeviceSamplesAccumulator*)h; }

const char* bcdcore_device_acc_error(void* h) { return ((DeviceSamplesAccumulator*)h)->lastError().c_str(); }

int bcdcore_device_acc_valid(void* h) { return ((DeviceSamplesAccumulator*)h)->isValid() ? 1 : 0; }

// samples: n x (line, col, r, g, b, weight) through addSample (left in the class's host batch until a call flushes it)
void bcdcore_device_acc_add(void* h, const float* s, long long n)
{
	DeviceSamplesAccumulator* a = (DeviceSamplesAccumulator*)h;
	for(long long i = 0; i < n; ++i, s += 6)
		a->addSample(int(s[0]), int(s[1]), s[2], s[3], s[4], s[5]);
}

// exportState into out[capacity]: the state's size, -1 on failure, -2 if capacity is too small (out == nullptr: the size only)
long long bcdcore_device_acc_export(void* h, unsigned char* out, long long capacity)
{
	std::vector<uint8_t> st;
	if(!((DeviceSamplesAccumulator*)h)->exportState(st)) return -1;
	if(!out) return (long long)st.size();
	if(capacity < (long long)st.size()) return -2;
	std::copy(st.begin(), st.end(), out);
	return (long long)st.size();
}

int bcdcore_device_acc_save(void* h, const char* path) { return ((DeviceSamplesAccumulator*)h)->saveState(path) ? 0 : -1; }
int bcdcore_device_acc_load(void* h, const char* path) { return ((DeviceSamplesAccumulator*)h)->loadState(path) ? 0 : -1; }
int bcdcore_device_acc_merge_state(void* h, const char* path) { return ((DeviceSamplesAccumulator*)h)->mergeState(path) ? 0 : -1; }
int bcdcore_device_acc_merge(void* dst, void* src)
{
	return ((DeviceSamplesAccumulator*)dst)->merge(*(const DeviceSamplesAccumulator*)src) ? 0 : -1;
}

// host snapshot (getSamplesStatistics) and the counters (lastError() keeps the message of an earlier refused call, so it is not checked)
int bcdcore_device_acc_statistics(void* h, float* ns, float* mean, float* cov, float* hist, long long* counts)
{
	DeviceSamplesAccumulator* a = (DeviceSamplesAccumulator*)h;
	if(!a->isValid()) return -1;
	SamplesStatisticsImages st = a->getSamplesStatistics();
	st.m_nbOfSamplesImage.copyDataTo(ns);
	st.m_meanImage.copyDataTo(mean);
	st.m_covarImage.copyDataTo(cov);
	st.m_histoImage.copyDataTo(hist);
	counts[0] = a->nbOfAccumulatedSamples();
	counts[1] = a->nbOfDroppedSamples();
	return 0;
}

void bcdcore_release_engines() { releaseEngines(); }

// runs bcd::Denoiser (nscales == 1) or bcd::MultiscaleDenoiser through the IDenoiser interface; returns denoise()'s bool.
// Null pointers are forwarded as null images to exercise the validation path.
/// The spike prefilter of the denoise_temporal* / denoise_sequence* wrappers, whose argument lists are fixed: what the calling thread's next such call sets on
/// its denoiser -- setSpikePrefilter(factor) when factor > 0 and setSpikePrefilterFrames(framesSwitch != 0).  The Python wrapper sets it ahead of the call and
/// puts it back to (0, 0) behind it; per thread, so that two threads' calls do not see each other's setting
static thread_local float t_prefilterFactor = 0.f;
static thread_local bool t_prefilterFramesSwitch = false;
void bcdcore_set_frame_prefilter(float factor, int framesSwitch) { t_prefilterFactor = factor; t_prefilterFramesSwitch = framesSwitch != 0; }
static void applyFramePrefilter(bcd::HipEngineSettings& io_rSettings)
{
	if(t_prefilterFactor > 0.f)
		io_rSettings.setSpikePrefilter(t_prefilterFactor);
	io_rSettings.setSpikePrefilterFrames(t_prefilterFramesSwitch);
}
static int g_lastProgressValues = 0;
/// number of distinct progress values the last bcdcore_denoise reported
int bcdcore_last_progress_values() { return g_lastProgressValues; }

static int g_lastNbOfCores = 0;
/// m_nbOfCores as the last bcdcore_denoise* left it in the denoiser's parameters (Denoiser.cpp:121 writes it back)
int bcdcore_last_nb_of_cores() { return g_lastNbOfCores; }

int bcdcore_denoise_ex(const float* col, const float* ns, const float* hist, const float* cov, int W, int H, int D, int nscales,
		float tau, int w, int b, float minEig, int randomOrder, float skipProbability, unsigned seed, float* out, int histWidthOverride,
		int useCuda, const int* devices, int nbOfDevices, float prefilterFactor);

int bcdcore_denoise(const float* col, const float* ns, const float* hist, const float* cov, int W, int H, int D, int nscales,
		float tau, int w, int b, float minEig, int randomOrder, float skipProbability, unsigned seed, float* out, int histWidthOverride)
{
	return bcdcore_denoise_ex(col, ns, hist, cov, W, H, D, nscales, tau, w, b, minEig, randomOrder, skipProbability, seed, out, histWidthOverride, 1, nullptr, 0, 0.f);
}

/// + DenoiserParameters::m_useCuda, HipEngineSettings::setDevices / setSpikePrefilter
int bcdcore_denoise_ex(const float* col, const float* ns, const float* hist, const float* cov, int W, int H, int D, int nscales,
		float tau, int w, int b, float minEig, int randomOrder, float skipProbability, unsigned seed, float* out, int histWidthOverride,
		int useCuda, const int* devices, int nbOfDevices, float prefilterFactor)
{
	Deepimf cImg, nImg, hImg, vImg, oImg(W > 0 ? W : 0, H > 0 ? H : 0, 3);
	DenoiserInputs in;
	if(col) { cImg.resize(W, H, 3); cImg.copyDataFrom(col); in.m_pColors = &cImg; }
	if(ns) { nImg.resize(W, H, 1); nImg.copyDataFrom(ns); in.m_pNbOfSamples = &nImg; }
	if(hist && histWidthOverride > 0) { hImg.resize(histWidthOverride, H, D); hImg.fill(0.f); in.m_pHistograms = &hImg; } // deliberately mismatched size
	else if(hist) { hImg.resize(W, H, D); hImg.copyDataFrom(hist); in.m_pHistograms = &hImg; }
	if(cov) { vImg.resize(W, H, 6); vImg.copyDataFrom(cov); in.m_pSampleCovariances = &vImg; }
	DenoiserOutputs o;
	o.m_pDenoisedColors = &oImg;
	DenoiserParameters p;
	p.m_histogramDistanceThreshold = tau; p.m_patchRadius = w; p.m_searchWindowRadius = b; p.m_minEigenValue = minEig;
	p.m_useRandomPixelOrder = randomOrder != 0; p.m_markedPixelsSkippingProbability = skipProbability;
	p.m_useCuda = useCuda != 0;
	std::unique_ptr<IDenoiser> d;
	HipEngineSettings* pSettings = nullptr;
	if(nscales > 1) { MultiscaleDenoiser* m = new MultiscaleDenoiser(nscales); pSettings = m; d.reset(m); }
	else { Denoiser* m = new Denoiser(); pSettings = m; d.reset(m); }
	pSettings->setOrderSeed(seed);
	if(devices && nbOfDevices > 0)
		pSettings->setDevices(std::vector<int>(devices, devices + nbOfDevices));
	pSettings->setSpikePrefilter(prefilterFactor);
	IDenoiser* pDenoiser = d.get();
	pDenoiser->setInputs(in);
	pDenoiser->setOutputs(o);
	pDenoiser->setParameters(p);
	float last = -1.f;
	bool monotone = true;
	int distinct = 0;
	pDenoiser->setProgressCallback([&](float f) { if(f < last) monotone = false; if(f != last) ++distinct; last = f; });
	const bool ok = pDenoiser->denoise();
	if(ok && out) oImg.copyDataTo(out);
	g_lastProgressValues = distinct;
	g_lastNbOfCores = pDenoiser->getParameters().m_nbOfCores;
	return ok ? (monotone ? 1 : 2) : 0;
}

/// bcd::Denoiser / bcd::MultiscaleDenoiser with setMomentSelection(true, varFloor): `nbOfLayers` colour layers as in bcdcore_denoise_layers_ex, sample counts,
/// and NO histogram image (DenoiserInputs::m_pHistograms stays null).  Returns denoise()'s bool
int bcdcore_denoise_moments(const float* cols, const float* covs, const float* ns, int W, int H, int nscales, int nbOfLayers, float tau, int b, float minEig,
		int randomOrder, float skipProbability, unsigned seed, int zeroBad, float prefilterFactor, int prefilterLayers, float varFloor, const int* devices,
		int nbOfDevices, float* outs)
{
	if(nbOfLayers < 1) return 0;
	const size_t np = size_t(W) * H;
	std::vector<Deepimf> c(nbOfLayers), v(nbOfLayers), o(nbOfLayers);
	for(int k = 0; k < nbOfLayers; ++k)
	{
		c[k].resize(W, H, 3); c[k].copyDataFrom(cols + k * np * 3);
		v[k].resize(W, H, 6); v[k].copyDataFrom(covs + k * np * 6);
		o[k].resize(W, H, 3);
	}
	Deepimf nImg(W, H, 1);
	nImg.copyDataFrom(ns);
	DenoiserInputs in;
	in.m_pColors = &c[0]; in.m_pNbOfSamples = &nImg; in.m_pSampleCovariances = &v[0];
	DenoiserOutputs out;
	out.m_pDenoisedColors = &o[0];
	DenoiserParameters p;
	p.m_histogramDistanceThreshold = tau; p.m_searchWindowRadius = b; p.m_minEigenValue = minEig;
	p.m_useRandomPixelOrder = randomOrder != 0; p.m_markedPixelsSkippingProbability = skipProbability;
	std::unique_ptr<IDenoiser> d;
	HipEngineSettings* pSettings = nullptr;
	if(nscales > 1) { MultiscaleDenoiser* m = new MultiscaleDenoiser(nscales); pSettings = m; d.reset(m); }
	else { Denoiser* m = new Denoiser(); pSettings = m; d.reset(m); }
	pSettings->setOrderSeed(seed);
	if(devices && nbOfDevices > 0)
		pSettings->setDevices(std::vector<int>(devices, devices + nbOfDevices));
	pSettings->setZeroBadOutputValues(zeroBad != 0);
	pSettings->setSpikePrefilter(prefilterFactor);
	pSettings->setSpikePrefilterLayers(prefilterLayers != 0);
	pSettings->setMomentSelection(true, varFloor);
	if(!pSettings->getMomentSelection() || pSettings->getMomentVarianceFloor() != varFloor)
		return 0;
	for(int k = 1; k < nbOfLayers; ++k)
		pSettings->addLayer(&c[k], &v[k], &o[k]);
	d->setInputs(in);
	d->setOutputs(out);
	d->setParameters(p);
	if(!d->denoise())
		return 0;
	for(int k = 0; k < nbOfLayers; ++k)
		o[k].copyDataTo(outs + k * np * 3);
	return 1;
}

/// bcd::Denoiser / bcd::MultiscaleDenoiser with setGuideFeatures(features, variances, floors, threshold): `nbOfLayers` colour layers as in
/// bcdcore_denoise_layers_ex; hist null: setMomentSelection(true, varFloor) and no histogram image.  features: W x H x nbOfChannels, null: a null features
/// pointer is set (the gate is off); variances: W x H x nbOfVarianceChannels or null; nbOfFloors floors; featureWidthOverride > 0: the feature image gets that width
/// (validation path).  Returns denoise()'s bool
int bcdcore_denoise_guided(const float* cols, const float* covs, const float* ns, const float* hist, int W, int H, int D, int nscales, int nbOfLayers, float tau,
		int b, float minEig, int randomOrder, float skipProbability, unsigned seed, int zeroBad, float prefilterFactor, int prefilterLayers, float varFloor,
		const float* features, const float* variances, int nbOfChannels, int nbOfVarianceChannels, const float* floors, int nbOfFloors, float threshold, int featureWidthOverride,
		const int* devices, int nbOfDevices, float* outs)
{
	if(nbOfLayers < 1) return 0;
	const size_t np = size_t(W) * H;
	std::vector<Deepimf> c(nbOfLayers), v(nbOfLayers), o(nbOfLayers);
	for(int k = 0; k < nbOfLayers; ++k)
	{
		c[k].resize(W, H, 3); c[k].copyDataFrom(cols + k * np * 3);
		v[k].resize(W, H, 6); v[k].copyDataFrom(covs + k * np * 6);
		o[k].resize(W, H, 3);
	}
	Deepimf nImg(W, H, 1), hImg, fImg, fvImg;
	nImg.copyDataFrom(ns);
	DenoiserInputs in;
	in.m_pColors = &c[0]; in.m_pNbOfSamples = &nImg; in.m_pSampleCovariances = &v[0];
	if(hist) { hImg.resize(W, H, D); hImg.copyDataFrom(hist); in.m_pHistograms = &hImg; }
	if(features && featureWidthOverride > 0) { fImg.resize(featureWidthOverride, H, nbOfChannels); fImg.fill(0.f); } // deliberately mismatched size
	else if(features) { fImg.resize(W, H, nbOfChannels); fImg.copyDataFrom(features); }
	if(variances) { fvImg.resize(W, H, nbOfVarianceChannels); fvImg.copyDataFrom(variances); }
	DenoiserOutputs out;
	out.m_pDenoisedColors = &o[0];
	DenoiserParameters p;
	p.m_histogramDistanceThreshold = tau; p.m_searchWindowRadius = b; p.m_minEigenValue = minEig;
	p.m_useRandomPixelOrder = randomOrder != 0; p.m_markedPixelsSkippingProbability = skipProbability;
	std::unique_ptr<IDenoiser> d;
	HipEngineSettings* pSettings = nullptr;
	if(nscales > 1) { MultiscaleDenoiser* m = new MultiscaleDenoiser(nscales); pSettings = m; d.reset(m); }
	else { Denoiser* m = new Denoiser(); pSettings = m; d.reset(m); }
	pSettings->setOrderSeed(seed);
	if(devices && nbOfDevices > 0)
		pSettings->setDevices(std::vector<int>(devices, devices + nbOfDevices));
	pSettings->setZeroBadOutputValues(zeroBad != 0);
	pSettings->setSpikePrefilter(prefilterFactor);
	pSettings->setSpikePrefilterLayers(prefilterLayers != 0);
	if(!hist)
		pSettings->setMomentSelection(true, varFloor);
	pSettings->setGuideFeatures(features ? &fImg : nullptr, variances ? &fvImg : nullptr, std::vector<float>(floors, floors + (floors ? nbOfFloors : 0)), threshold);
	if((pSettings->getGuideFeatures() != nullptr) != (features != nullptr) || pSettings->getGuideThreshold() != threshold || int(pSettings->getGuideFloors().size()) != (floors ? nbOfFloors : 0))
		return 0;
	for(int k = 1; k < nbOfLayers; ++k)
		pSettings->addLayer(&c[k], &v[k], &o[k]);
	d->setInputs(in);
	d->setOutputs(out);
	d->setParameters(p);
	if(!d->denoise())
		return 0;
	for(int k = 0; k < nbOfLayers; ++k)
		o[k].copyDataTo(outs + k * np * 3);
	return 1;
}

/// bcd::Denoiser / bcd::MultiscaleDenoiser with `nbOfLayers` colour layers: layer 0 through DenoiserInputs / DenoiserOutputs, the others through
/// addLayer.  cols / covs / outs: nbOfLayers images one behind the other.  sizeMismatchLayer > 0: that added layer gets a covariance image one
/// line short (validation path).  afterClear != 0: clearLayers() and a second denoise() into outs[0] must still succeed.  Returns denoise()'s bool
/// prefilterLayers != 0: setSpikePrefilterLayers(true) -- the prefilter is accepted beside added layers and covers every layer
int bcdcore_denoise_layers_ex(const float* cols, const float* covs, const float* ns, const float* hist, int W, int H, int D, int nscales, int nbOfLayers,
		float tau, int b, float minEig, int randomOrder, float skipProbability, unsigned seed, int zeroBad, float prefilterFactor, int sizeMismatchLayer,
		int afterClear, int prefilterLayers, float* outs)
{
	if(nbOfLayers < 1) return 0;
	const size_t np = size_t(W) * H;
	std::vector<Deepimf> c(nbOfLayers), v(nbOfLayers), o(nbOfLayers);
	for(int k = 0; k < nbOfLayers; ++k)
	{
		c[k].resize(W, H, 3); c[k].copyDataFrom(cols + k * np * 3);
		if(k > 0 && k == sizeMismatchLayer) { v[k].resize(W, H - 1, 6); v[k].fill(0.f); }
		else { v[k].resize(W, H, 6); v[k].copyDataFrom(covs + k * np * 6); }
		o[k].resize(W, H, 3);
	}
	Deepimf nImg(W, H, 1), hImg(W, H, D);
	nImg.copyDataFrom(ns); hImg.copyDataFrom(hist);
	DenoiserInputs in;
	in.m_pColors = &c[0]; in.m_pNbOfSamples = &nImg; in.m_pHistograms = &hImg; in.m_pSampleCovariances = &v[0];
	DenoiserOutputs out;
	out.m_pDenoisedColors = &o[0];
	DenoiserParameters p;
	p.m_histogramDistanceThreshold = tau; p.m_searchWindowRadius = b; p.m_minEigenValue = minEig;
	p.m_useRandomPixelOrder = randomOrder != 0; p.m_markedPixelsSkippingProbability = skipProbability;
	std::unique_ptr<IDenoiser> d;
	HipEngineSettings* pSettings = nullptr;
	if(nscales > 1) { MultiscaleDenoiser* m = new MultiscaleDenoiser(nscales); pSettings = m; d.reset(m); }
	else { Denoiser* m = new Denoiser(); pSettings = m; d.reset(m); }
	pSettings->setOrderSeed(seed);
	pSettings->setZeroBadOutputValues(zeroBad != 0);
	pSettings->setSpikePrefilter(prefilterFactor);
	pSettings->setSpikePrefilterLayers(prefilterLayers != 0);
	for(int k = 1; k < nbOfLayers; ++k)
		pSettings->addLayer(&c[k], &v[k], &o[k]);
	d->setInputs(in);
	d->setOutputs(out);
	d->setParameters(p);
	if(!d->denoise())
		return 0;
	for(int k = 0; k < nbOfLayers; ++k)
		o[k].copyDataTo(outs + k * np * 3);
	if(afterClear)
	{
		pSettings->clearLayers();
		o[0] = c[0];
		if(!pSettings->getLayers().empty() || !d->denoise())
			return 0;
		o[0].copyDataTo(outs);
	}
	return 1;
}

int bcdcore_denoise_layers(const float* cols, const float* covs, const float* ns, const float* hist, int W, int H, int D, int nscales, int nbOfLayers,
		float tau, int b, float minEig, int randomOrder, float skipProbability, unsigned seed, int zeroBad, float prefilterFactor, int sizeMismatchLayer,
		int afterClear, float* outs)
{
	return bcdcore_denoise_layers_ex(cols, covs, ns, hist, W, H, D, nscales, nbOfLayers, tau, b, minEig, randomOrder, skipProbability, seed, zeroBad, prefilterFactor,
			sizeMismatchLayer, afterClear, 0, outs);
}

/// bcd::Denoiser / bcd::MultiscaleDenoiser with neighbouring frames of the sequence (addNeighbourFrame): nbCols etc. hold nbOfNeighbours images one behind
/// the other.  afterClear != 0: clearNeighbourFrames() and a second denoise() follow, whose result replaces the first.  Returns denoise()'s bool.
/// motions: null, or nbOfNeighbours motion fields (W x H x 2) one behind the other, of which neighbour k's is handed to setNeighbourMotion when hasMotion[k] != 0
static int denoiseTemporal(const float* col, const float* ns, const float* hist, const float* cov, const float* nbCols, const float* nbNs, const float* nbHists,
		const float* nbCovs, int nbOfNeighbours, const float* motions, const int* hasMotion, int W, int H, int D, int nscales, float tau, int b, float minEig, int randomOrder,
		float skipProbability, unsigned seed, int afterClear, float* out)
{
	Deepimf cImg(W, H, 3), nImg(W, H, 1), hImg(W, H, D), vImg(W, H, 6), oImg(W, H, 3);
	cImg.copyDataFrom(col); nImg.copyDataFrom(ns); hImg.copyDataFrom(hist); vImg.copyDataFrom(cov);
	std::vector<Deepimf> c(nbOfNeighbours), n(nbOfNeighbours), h(nbOfNeighbours), v(nbOfNeighbours), mv(nbOfNeighbours);
	const size_t npix = size_t(W) * H;
	DenoiserInputs in;
	in.m_pColors = &cImg; in.m_pNbOfSamples = &nImg; in.m_pHistograms = &hImg; in.m_pSampleCovariances = &vImg;
	DenoiserOutputs o;
	o.m_pDenoisedColors = &oImg;
	DenoiserParameters p;
	p.m_histogramDistanceThreshold = tau;
	p.m_searchWindowRadius = b;
	p.m_minEigenValue = minEig;
	p.m_useRandomPixelOrder = randomOrder != 0;
	p.m_markedPixelsSkippingProbability = skipProbability;
	std::unique_ptr<MultiscaleDenoiser> multi;
	std::unique_ptr<Denoiser> mono;
	IDenoiser* d;
	HipEngineSettings* pSettings;
	if(nscales > 1) { multi.reset(new MultiscaleDenoiser(nscales)); d = multi.get(); pSettings = multi.get(); }
	else { mono.reset(new Denoiser()); d = mono.get(); pSettings = mono.get(); }
	pSettings->setOrderSeed(seed);
	applyFramePrefilter(*pSettings);
	for(int k = 0; k < nbOfNeighbours; ++k)
	{
		c[k].resize(W, H, 3); n[k].resize(W, H, 1); h[k].resize(W, H, D); v[k].resize(W, H, 6);
		c[k].copyDataFrom(nbCols + k * npix * 3); n[k].copyDataFrom(nbNs + k * npix); h[k].copyDataFrom(nbHists + k * npix * D); v[k].copyDataFrom(nbCovs + k * npix * 6);
		DenoiserInputs f;
		f.m_pColors = &c[k]; f.m_pNbOfSamples = &n[k]; f.m_pHistograms = &h[k]; f.m_pSampleCovariances = &v[k];
		pSettings->addNeighbourFrame(f);
		if(motions && hasMotion[k])
		{
			mv[k].resize(W, H, 2);
			mv[k].copyDataFrom(motions + k * npix * 2);
			pSettings->setNeighbourMotion(size_t(k), &mv[k]);
		}
	}
	d->setInputs(in);
	d->setOutputs(o);
	d->setParameters(p);
	oImg = cImg; // (the multiscale path wants the output pre-sized like the input)
	bool ok = d->denoise();
	if(ok && afterClear)
	{
		pSettings->clearNeighbourFrames();
		oImg = cImg;
		ok = d->denoise();
	}
	if(ok) oImg.copyDataTo(out);
	return ok ? 1 : 0;
}

int bcdcore_denoise_temporal(const float* col, const float* ns, const float* hist, const float* cov, const float* nbCols, const float* nbNs, const float* nbHists,
		const float* nbCovs, int nbOfNeighbours, int W, int H, int D, int nscales, float tau, int b, float minEig, int randomOrder, float skipProbability, unsigned seed,
		int afterClear, float* out)
{
	return denoiseTemporal(col, ns, hist, cov, nbCols, nbNs, nbHists, nbCovs, nbOfNeighbours, nullptr, nullptr, W, H, D, nscales, tau, b, minEig, randomOrder, skipProbability,
			seed, afterClear, out);
}

/// ... with motion fields (setNeighbourMotion): motions holds nbOfNeighbours fields of W x H x 2 one behind the other, hasMotion[k] == 0 leaves neighbour k without
int bcdcore_denoise_temporal_motion(const float* col, const float* ns, const float* hist, const float* cov, const float* nbCols, const float* nbNs, const float* nbHists,
		const float* nbCovs, int nbOfNeighbours, const float* motions, const int* hasMotion, int W, int H, int D, int nscales, float tau, int b, float minEig, int randomOrder,
		float skipProbability, unsigned seed, int afterClear, float* out)
{
	return denoiseTemporal(col, ns, hist, cov, nbCols, nbNs, nbHists, nbCovs, nbOfNeighbours, motions, hasMotion, W, H, D, nscales, tau, b, minEig, randomOrder,
			skipProbability, seed, afterClear, out);
}

/// bcd::SequenceDenoiser over nbOfFrames frames held one behind the other in cols / nss / hists / covs: every frame is pushed, popped as soon as it is ready
/// (after end() for the last ones) and written to outs in frame order.  unsupported: settings a sequence must refuse before any device is asked for -- bit 0
/// addLayer, bit 1 addNeighbourFrame, bit 2 setMomentSelection(true), bit 3 setSpikePrefilter(2), bit 4 two devices, bit 5 a second frame of another size.
/// Returns 1 when every push and pop succeeded and the frames came in order, else 0.
int bcdcore_denoise_sequence(const float* cols, const float* nss, const float* hists, const float* covs, int nbOfFrames, int W, int H, int D, int nscales, int radius,
		float tau, int w, int b, float minEig, int randomOrder, float skipProbability, unsigned seed, int unsupported, float* outs)
{
	const size_t npix = size_t(W) * H;
	SequenceDenoiser sequence(nscales, radius);
	DenoiserParameters p;
	p.m_histogramDistanceThreshold = tau;
	p.m_patchRadius = w;
	p.m_searchWindowRadius = b;
	p.m_minEigenValue = minEig;
	p.m_useRandomPixelOrder = randomOrder != 0;
	p.m_markedPixelsSkippingProbability = skipProbability;
	sequence.setParameters(p);
	sequence.setOrderSeed(seed);
	applyFramePrefilter(sequence);
	Deepimf extra(W, H, 3), extraCov(W, H, 6), extraOut;
	DenoiserInputs extraFrame;
	if(unsupported & 1) sequence.addLayer(&extra, &extraCov, &extraOut);
	if(unsupported & 2) sequence.addNeighbourFrame(extraFrame);
	if(unsupported & 4) sequence.setMomentSelection(true);
	if(unsupported & 8) sequence.setSpikePrefilter(2.f);
	if(unsupported & 16) sequence.setDevices(std::vector<int>{ 0, 1 });
	int popped = 0;
	auto popReady = [&]() -> bool
	{
		while(sequence.ready() > 0)
		{
			Deepimf out;
			DenoiserOutputs o;
			o.m_pDenoisedColors = &out;
			if(!sequence.popFrame(o) || sequence.getLastFrameIndex() != popped || out.getWidth() != W || out.getHeight() != H || out.getDepth() != 3)
				return false;
			out.copyDataTo(outs + size_t(popped) * npix * 3);
			++popped;
		}
		return true;
	};
	for(int k = 0; k < nbOfFrames; ++k)
	{
		const bool otherSize = (unsupported & 32) && k == 1;
		const int wk = otherSize ? W - 1 : W;
		Deepimf c(wk, H, 3), n(wk, H, 1), h(wk, H, D), v(wk, H, 6);
		if(!otherSize)
		{
			c.copyDataFrom(cols + k * npix * 3); n.copyDataFrom(nss + k * npix); h.copyDataFrom(hists + k * npix * D); v.copyDataFrom(covs + k * npix * 6);
		}
		DenoiserInputs f;
		f.m_pColors = &c; f.m_pNbOfSamples = &n; f.m_pHistograms = &h; f.m_pSampleCovariances = &v;
		if(!sequence.pushFrame(f))
			return 0;
		if(k == nbOfFrames - 1 && !sequence.end())
			return 0;
		if(!popReady())
			return 0;
	}
	return popped == nbOfFrames ? 1 : 0;
}

/// bcd::SequenceDenoiser with setFrameSettings(true): per frame nbOfLayers layers (cols / covs frame-major, layer 0 the DenoiserInputs images; outs the same
/// way), histograms (hists null: setMomentSelection(true, varFloor), D is not looked at) and nbOfChannels feature channels (features null: no gate; variances
/// null: none) with nbOfFloors floors and the threshold.  break_: settings the class must refuse before a device is asked for -- bit 0 addNeighbourFrame, bit 1
/// the spike prefilter, bit 2 two devices, bit 3 the second frame with one layer fewer, bit 4 the second frame without its variances (or, without variances,
/// without its features), bit 5 no layer registered when the first frame is popped.  Returns 1 when every push and pop succeeded in order, else 0.
/// motions (bcdcore_denoise_sequence_motion; null: no frame brings a field): per frame two W x H x 2 fields one behind the other, towards the frame before and
/// after it, hasMotion 2 flags per frame (0: nullptr for that field) -> setFrameMotion ahead of every push.  breakMotion: what pushFrame must refuse before a
/// device is asked for -- bit 0 the first field given has 3 channels, bit 1 it is one pixel narrower than the frame.
static int denoiseSequenceModes(const float* cols, const float* nss, const float* hists, const float* covs, const float* features, const float* variances, int nbOfFrames,
		int nbOfLayers, int nbOfChannels, const float* floors, int nbOfFloors, float threshold, float varFloor, int W, int H, int D, int nscales, int radius, float tau,
		int w, int b, float minEig, int randomOrder, float skipProbability, unsigned seed, int break_, float* outs, const float* motions, const int* hasMotion,
		int breakMotion)
{
	const size_t npix = size_t(W) * H;
	SequenceDenoiser sequence(nscales, radius);
	DenoiserParameters p;
	p.m_histogramDistanceThreshold = tau;
	p.m_patchRadius = w;
	p.m_searchWindowRadius = b;
	p.m_minEigenValue = minEig;
	p.m_useRandomPixelOrder = randomOrder != 0;
	p.m_markedPixelsSkippingProbability = skipProbability;
	sequence.setParameters(p);
	sequence.setOrderSeed(seed);
	applyFramePrefilter(sequence);
	sequence.setFrameSettings(true);
	if(!hists) sequence.setMomentSelection(true, varFloor);
	DenoiserInputs extraFrame;
	if(break_ & 1) sequence.addNeighbourFrame(extraFrame);
	if(break_ & 2) sequence.setSpikePrefilter(2.f);
	if(break_ & 4) sequence.setDevices(std::vector<int>{ 0, 1 });
	const std::vector<float> floorList(floors, floors + (floors ? nbOfFloors : 0));
	const int L = nbOfLayers;
	int popped = 0;
	std::vector<Deepimf> layerOuts(L > 1 ? L - 1 : 0);
	std::vector<Deepimf> lc, lv;
	Deepimf feat, var;
	auto registerLayers = [&](int n)
	{
		sequence.clearLayers();
		for(int k = 1; k < n; ++k) sequence.addLayer(&lc[k - 1], &lv[k - 1], &layerOuts[k - 1]);
	};
	auto popReady = [&]() -> bool
	{
		while(sequence.ready() > 0)
		{
			Deepimf out;
			DenoiserOutputs o;
			o.m_pDenoisedColors = &out;
			if((break_ & 32) && popped == 0) sequence.clearLayers();
			if(!sequence.popFrame(o) || sequence.getLastFrameIndex() != popped || out.getWidth() != W || out.getHeight() != H || out.getDepth() != 3)
				return false;
			out.copyDataTo(outs + (size_t(popped) * L) * npix * 3);
			for(int k = 1; k < L; ++k)
			{
				if(layerOuts[k - 1].getWidth() != W || layerOuts[k - 1].getHeight() != H || layerOuts[k - 1].getDepth() != 3) return false;
				layerOuts[k - 1].copyDataTo(outs + (size_t(popped) * L + k) * npix * 3);
			}
			++popped;
		}
		return true;
	};
	for(int f = 0; f < nbOfFrames; ++f)
	{
		Deepimf c(W, H, 3), n(W, H, 1), h, v(W, H, 6);
		c.copyDataFrom(cols + (size_t(f) * L) * npix * 3); n.copyDataFrom(nss + f * npix); v.copyDataFrom(covs + (size_t(f) * L) * npix * 6);
		if(hists) { h = Deepimf(W, H, D); h.copyDataFrom(hists + f * npix * D); }
		lc.assign(L - 1, Deepimf(W, H, 3)); lv.assign(L - 1, Deepimf(W, H, 6));
		for(int k = 1; k < L; ++k) { lc[k - 1].copyDataFrom(cols + (size_t(f) * L + k) * npix * 3); lv[k - 1].copyDataFrom(covs + (size_t(f) * L + k) * npix * 6); }
		registerLayers((break_ & 8) && f == 1 ? L - 1 : L);
		if(features)
		{
			const bool drop = (break_ & 16) && f == 1;
			feat = Deepimf(W, H, nbOfChannels); feat.copyDataFrom(features + f * npix * nbOfChannels);
			if(variances) { var = Deepimf(W, H, nbOfChannels); var.copyDataFrom(variances + f * npix * nbOfChannels); }
			sequence.setGuideFeatures(drop && !variances ? nullptr : &feat, variances && !drop ? &var : nullptr, floorList, threshold);
		}
		DenoiserInputs in;
		in.m_pColors = &c; in.m_pNbOfSamples = &n; in.m_pHistograms = hists ? &h : nullptr; in.m_pSampleCovariances = &v;
		Deepimf field[2];
		for(int d = 0; motions && d < 2; ++d)
		{
			if(!hasMotion[2 * f + d]) continue;
			if(breakMotion)
			{
				field[d] = Deepimf((breakMotion & 2) ? W - 1 : W, H, (breakMotion & 1) ? 3 : 2);
				breakMotion = 0;
				continue;
			}
			field[d] = Deepimf(W, H, 2);
			field[d].copyDataFrom(motions + (size_t(f) * 2 + d) * npix * 2);
		}
		if(motions) sequence.setFrameMotion(field[0].isEmpty() ? nullptr : &field[0], field[1].isEmpty() ? nullptr : &field[1]);
		if(!sequence.pushFrame(in))
			return 0;
		if(f == nbOfFrames - 1 && !sequence.end())
			return 0;
		registerLayers(L);
		if(!popReady())
			return 0;
	}
	return popped == nbOfFrames ? 1 : 0;
}

int bcdcore_denoise_sequence_modes(const float* cols, const float* nss, const float* hists, const float* covs, const float* features, const float* variances, int nbOfFrames,
		int nbOfLayers, int nbOfChannels, const float* floors, int nbOfFloors, float threshold, float varFloor, int W, int H, int D, int nscales, int radius, float tau,
		int w, int b, float minEig, int randomOrder, float skipProbability, unsigned seed, int break_, float* outs)
{
	return denoiseSequenceModes(cols, nss, hists, covs, features, variances, nbOfFrames, nbOfLayers, nbOfChannels, floors, nbOfFloors, threshold, varFloor, W, H, D, nscales,
			radius, tau, w, b, minEig, randomOrder, skipProbability, seed, break_, outs, nullptr, nullptr, 0);
}

/// bcdcore_denoise_sequence_modes with per-step motion fields (SequenceDenoiser::setFrameMotion), see denoiseSequenceModes
int bcdcore_denoise_sequence_motion(const float* cols, const float* nss, const float* hists, const float* covs, const float* features, const float* variances, int nbOfFrames,
		int nbOfLayers, int nbOfChannels, const float* floors, int nbOfFloors, float threshold, float varFloor, int W, int H, int D, int nscales, int radius, float tau,
		int w, int b, float minEig, int randomOrder, float skipProbability, unsigned seed, int break_, float* outs, const float* motions, const int* hasMotion,
		int breakMotion)
{
	return denoiseSequenceModes(cols, nss, hists, covs, features, variances, nbOfFrames, nbOfLayers, nbOfChannels, floors, nbOfFloors, threshold, varFloor, W, H, D, nscales,
			radius, tau, w, b, minEig, randomOrder, skipProbability, seed, break_, outs, motions, hasMotion, breakMotion);
}

/// bcd::Denoiser / bcd::MultiscaleDenoiser with neighbouring frames AND colour layers (addLayer, addNeighbourFrame, addNeighbourFrameLayer).  cols / covs hold
/// nbOfLayers images of the frame one behind the other (layer 0 = the primary images), nbCols / nbCovs nbOfNeighbours x nbOfLayers images (neighbour-major),
/// nbNs / nbHists one image per neighbour.  The last neighbour gets dropLayers fewer layers than the frame (> 0: denoise() must refuse).  afterClear != 0:
/// clearNeighbourFrames() and a second denoise() follow (the plain layered call), whose results replace the first.  Returns denoise()'s bool.
/// i_pGuide (bcdcore_denoise_temporal_guided): setGuideFeatures on the frame and setNeighbourGuideFeatures on the first nbOfNeighboursWithFeatures neighbours --
/// features W x H x nbOfChannels, the neighbours' W x H x nbOfNeighbourChannels one behind the other, variances of the same sizes or null --, and the settings
/// the combination must refuse: momentSelection != 0 -> setMomentSelection(true), nbOfDevices > 0 -> setDevices.
struct TemporalGuide
{
	const float* features; const float* variances; int nbOfChannels; const float* floors; int nbOfFloors; float threshold;
	const float* nbFeatures; const float* nbVariances; int nbOfNeighbourChannels; int nbOfNeighboursWithFeatures;
	int momentSelection; const int* devices; int nbOfDevices;
};

static int denoiseTemporalLayers(const float* cols, const float* covs, const float* ns, const float* hist, const float* nbCols, const float* nbCovs, const float* nbNs,
		const float* nbHists, int nbOfNeighbours, int nbOfLayers, const float* motions, const int* hasMotion, int W, int H, int D, int nscales, float tau, int b, float minEig,
		int randomOrder, float skipProbability, unsigned seed, int dropLayers, int afterClear, float* outs, const TemporalGuide* i_pGuide = nullptr)
{
	const size_t npix = size_t(W) * H;
	Deepimf nImg(W, H, 1), hImg(W, H, D);
	nImg.copyDataFrom(ns); hImg.copyDataFrom(hist);
	std::vector<Deepimf> c(nbOfLayers), v(nbOfLayers), o(nbOfLayers);
	for(int k = 0; k < nbOfLayers; ++k)
	{
		c[k].resize(W, H, 3); v[k].resize(W, H, 6);
		c[k].copyDataFrom(cols + k * npix * 3); v[k].copyDataFrom(covs + k * npix * 6);
		o[k] = c[k]; // (the multiscale path wants the output pre-sized like the input)
	}
	std::vector<Deepimf> fn(nbOfNeighbours), fh(nbOfNeighbours), fc(size_t(nbOfNeighbours) * nbOfLayers), fv(size_t(nbOfNeighbours) * nbOfLayers), mv(nbOfNeighbours);
	DenoiserInputs in;
	in.m_pColors = &c[0]; in.m_pNbOfSamples = &nImg; in.m_pHistograms = &hImg; in.m_pSampleCovariances = &v[0];
	DenoiserOutputs out;
	out.m_pDenoisedColors = &o[0];
	DenoiserParameters p;
	p.m_histogramDistanceThreshold = tau;
	p.m_searchWindowRadius = b;
	p.m_minEigenValue = minEig;
	p.m_useRandomPixelOrder = randomOrder != 0;
	p.m_markedPixelsSkippingProbability = skipProbability;
	std::unique_ptr<MultiscaleDenoiser> multi;
	std::unique_ptr<Denoiser> mono;
	IDenoiser* d;
	HipEngineSettings* pSettings;
	if(nscales > 1) { multi.reset(new MultiscaleDenoiser(nscales)); d = multi.get(); pSettings = multi.get(); }
	else { mono.reset(new Denoiser()); d = mono.get(); pSettings = mono.get(); }
	pSettings->setOrderSeed(seed);
	applyFramePrefilter(*pSettings);
	for(int k = 1; k < nbOfLayers; ++k)
		pSettings->addLayer(&c[k], &v[k], &o[k]);
	for(int f = 0; f < nbOfNeighbours; ++f)
	{
		fn[f].resize(W, H, 1); fh[f].resize(W, H, D);
		fn[f].copyDataFrom(nbNs + f * npix); fh[f].copyDataFrom(nbHists + f * npix * D);
		for(int k = 0; k < nbOfLayers; ++k)
		{
			const size_t i = size_t(f) * nbOfLayers + k;
			fc[i].resize(W, H, 3); fv[i].resize(W, H, 6);
			fc[i].copyDataFrom(nbCols + i * npix * 3); fv[i].copyDataFrom(nbCovs + i * npix * 6);
		}
		DenoiserInputs frame;
		frame.m_pColors = &fc[size_t(f) * nbOfLayers]; frame.m_pNbOfSamples = &fn[f]; frame.m_pHistograms = &fh[f]; frame.m_pSampleCovariances = &fv[size_t(f) * nbOfLayers];
		pSettings->addNeighbourFrame(frame);
		const int given = nbOfLayers - (f == nbOfNeighbours - 1 ? dropLayers : 0);
		for(int k = 1; k < given; ++k)
			pSettings->addNeighbourFrameLayer(size_t(f), &fc[size_t(f) * nbOfLayers + k], &fv[size_t(f) * nbOfLayers + k]);
		if(motions && hasMotion[f])
		{
			mv[f].resize(W, H, 2);
			mv[f].copyDataFrom(motions + f * npix * 2);
			pSettings->setNeighbourMotion(size_t(f), &mv[f]);
		}
	}
	Deepimf gf, gv;
	std::vector<Deepimf> nf(nbOfNeighbours), nv(nbOfNeighbours);
	if(i_pGuide)
	{
		const TemporalGuide& g = *i_pGuide;
		gf.resize(W, H, g.nbOfChannels); gf.copyDataFrom(g.features);
		if(g.variances) { gv.resize(W, H, g.nbOfChannels); gv.copyDataFrom(g.variances); }
		pSettings->setGuideFeatures(&gf, g.variances ? &gv : nullptr, std::vector<float>(g.floors, g.floors + g.nbOfFloors), g.threshold);
		for(int f = 0; f < nbOfNeighbours && f < g.nbOfNeighboursWithFeatures; ++f)
		{
			const size_t n = npix * g.nbOfNeighbourChannels;
			nf[f].resize(W, H, g.nbOfNeighbourChannels); nf[f].copyDataFrom(g.nbFeatures + f * n);
			if(g.nbVariances) { nv[f].resize(W, H, g.nbOfNeighbourChannels); nv[f].copyDataFrom(g.nbVariances + f * n); }
			pSettings->setNeighbourGuideFeatures(size_t(f), &nf[f], g.nbVariances ? &nv[f] : nullptr);
		}
		if(g.momentSelection)
			pSettings->setMomentSelection(true);
		if(g.devices && g.nbOfDevices > 0)
			pSettings->setDevices(std::vector<int>(g.devices, g.devices + g.nbOfDevices));
	}
	d->setInputs(in);
	d->setOutputs(out);
	d->setParameters(p);
	bool ok = d->denoise();
	if(ok && afterClear)
	{
		pSettings->clearNeighbourFrames();
		for(int k = 0; k < nbOfLayers; ++k)
			o[k] = c[k];
		ok = d->denoise();
	}
	if(ok)
		for(int k = 0; k < nbOfLayers; ++k)
			o[k].copyDataTo(outs + k * npix * 3);
	return ok ? 1 : 0;
}

int bcdcore_denoise_temporal_layers(const float* cols, const float* covs, const float* ns, const float* hist, const float* nbCols, const float* nbCovs, const float* nbNs,
		const float* nbHists, int nbOfNeighbours, int nbOfLayers, int W, int H, int D, int nscales, float tau, int b, float minEig, int randomOrder,
		float skipProbability, unsigned seed, int dropLayers, int afterClear, float* outs)
{
	return denoiseTemporalLayers(cols, covs, ns, hist, nbCols, nbCovs, nbNs, nbHists, nbOfNeighbours, nbOfLayers, nullptr, nullptr, W, H, D, nscales, tau, b, minEig,
			randomOrder, skipProbability, seed, dropLayers, afterClear, outs);
}

/// ... with motion fields, as bcdcore_denoise_temporal_motion takes them
int bcdcore_denoise_temporal_layers_motion(const float* cols, const float* covs, const float* ns, const float* hist, const float* nbCols, const float* nbCovs,
		const float* nbNs, const float* nbHists, int nbOfNeighbours, int nbOfLayers, const float* motions, const int* hasMotion, int W, int H, int D, int nscales, float tau,
		int b, float minEig, int randomOrder, float skipProbability, unsigned seed, int dropLayers, int afterClear, float* outs)
{
	return denoiseTemporalLayers(cols, covs, ns, hist, nbCols, nbCovs, nbNs, nbHists, nbOfNeighbours, nbOfLayers, motions, hasMotion, W, H, D, nscales, tau, b, minEig,
			randomOrder, skipProbability, seed, dropLayers, afterClear, outs);
}

/// ... with feature buffers on the frame (setGuideFeatures) and on the neighbours (setNeighbourGuideFeatures): see TemporalGuide.  motions may be null
int bcdcore_denoise_temporal_guided(const float* cols, const float* covs, const float* ns, const float* hist, const float* nbCols, const float* nbCovs, const float* nbNs,
		const float* nbHists, int nbOfNeighbours, int nbOfLayers, const float* motions, const int* hasMotion, int W, int H, int D, int nscales, float tau, int b, float minEig,
		int randomOrder, float skipProbability, unsigned seed, int afterClear, const float* features, const float* variances, int nbOfChannels, const float* floors,
		int nbOfFloors, float threshold, const float* nbFeatures, const float* nbVariances, int nbOfNeighbourChannels, int nbOfNeighboursWithFeatures, int momentSelection,
		const int* devices, int nbOfDevices, float* outs)
{
	if(!features || !floors || nbOfChannels < 1 || nbOfNeighbourChannels < 1) return 0;
	const TemporalGuide guide = { features, variances, nbOfChannels, floors, nbOfFloors, threshold, nbFeatures, nbVariances, nbOfNeighbourChannels,
			nbFeatures ? nbOfNeighboursWithFeatures : 0, momentSelection, devices, nbOfDevices };
	return denoiseTemporalLayers(cols, covs, ns, hist, nbCols, nbCovs, nbNs, nbHists, nbOfNeighbours, nbOfLayers, motions, hasMotion, W, H, D, nscales, tau, b, minEig,
			randomOrder, skipProbability, seed, 0, afterClear, outs, &guide);
}

/// bcd::Denoiser / bcd::MultiscaleDenoiser under setMomentSelection(true) with neighbour frames added by addNeighbourFrameMoments (no histogram anywhere):
/// cols / covs hold nbOfLayers images of the frame (layer 0 = the primary images), nbCols / nbCovs nbOfNeighbours x nbOfLayers images (neighbour-major), nbNs one
/// image per neighbour; motions / hasMotion as bcdcore_denoise_temporal_motion takes them (motions may be null); features null: no feature gate, else as
/// bcdcore_denoise_temporal_guided (every neighbour gets its feature buffers).  For the refusals denoise() owes: momentSelection == 0 leaves setMomentSelection
/// off, the first nbOfPlainNeighbours neighbours are added by addNeighbourFrame (with a histogram image of ones), the last neighbour gets dropLayers fewer
/// layers than the frame, nbOfDevices > 0 -> setDevices.  Returns denoise()'s bool.
int bcdcore_denoise_temporal_moments(const float* cols, const float* covs, const float* ns, const float* nbCols, const float* nbCovs, const float* nbNs, int nbOfNeighbours,
		int nbOfLayers, const float* motions, const int* hasMotion, int W, int H, int nscales, float tau, int b, float minEig, int randomOrder, float skipProbability,
		unsigned seed, float varianceFloor, const float* features, const float* variances, int nbOfChannels, const float* floors, int nbOfFloors, float threshold,
		const float* nbFeatures, const float* nbVariances, int momentSelection, int nbOfPlainNeighbours, int dropLayers, const int* devices, int nbOfDevices, float* outs)
{
	if(nbOfLayers < 1 || nbOfNeighbours < 0 || (features && (!floors || nbOfChannels < 1 || (nbOfNeighbours > 0 && !nbFeatures)))) return 0;
	const size_t npix = size_t(W) * H;
	Deepimf nImg(W, H, 1), ones(W, H, 12);
	nImg.copyDataFrom(ns);
	ones.fill(1.f);
	std::vector<Deepimf> c(nbOfLayers), v(nbOfLayers), o(nbOfLayers);
	for(int k = 0; k < nbOfLayers; ++k)
	{
		c[k].resize(W, H, 3); v[k].resize(W, H, 6);
		c[k].copyDataFrom(cols + k * npix * 3); v[k].copyDataFrom(covs + k * npix * 6);
		o[k] = c[k]; // (the multiscale path wants the output pre-sized like the input)
	}
	std::vector<Deepimf> fn(nbOfNeighbours), fc(size_t(nbOfNeighbours) * nbOfLayers), fv(size_t(nbOfNeighbours) * nbOfLayers), mv(nbOfNeighbours), nf(nbOfNeighbours), nv(nbOfNeighbours);
	DenoiserInputs in;
	in.m_pColors = &c[0]; in.m_pNbOfSamples = &nImg; in.m_pHistograms = nullptr; in.m_pSampleCovariances = &v[0];
	DenoiserOutputs out;
	out.m_pDenoisedColors = &o[0];
	DenoiserParameters p;
	p.m_histogramDistanceThreshold = tau;
	p.m_searchWindowRadius = b;
	p.m_minEigenValue = minEig;
	p.m_useRandomPixelOrder = randomOrder != 0;
	p.m_markedPixelsSkippingProbability = skipProbability;
	std::unique_ptr<MultiscaleDenoiser> multi;
	std::unique_ptr<Denoiser> mono;
	IDenoiser* d;
	HipEngineSettings* pSettings;
	if(nscales > 1) { multi.reset(new MultiscaleDenoiser(nscales)); d = multi.get(); pSettings = multi.get(); }
	else { mono.reset(new Denoiser()); d = mono.get(); pSettings = mono.get(); }
	pSettings->setOrderSeed(seed);
	applyFramePrefilter(*pSettings);
	if(momentSelection)
		pSettings->setMomentSelection(true, varianceFloor);
	else
		in.m_pHistograms = &ones;
	for(int k = 1; k < nbOfLayers; ++k)
		pSettings->addLayer(&c[k], &v[k], &o[k]);
	Deepimf gf, gv;
	if(features)
	{
		gf.resize(W, H, nbOfChannels); gf.copyDataFrom(features);
		if(variances) { gv.resize(W, H, nbOfChannels); gv.copyDataFrom(variances); }
		pSettings->setGuideFeatures(&gf, variances ? &gv : nullptr, std::vector<float>(floors, floors + nbOfFloors), threshold);
	}
	for(int f = 0; f < nbOfNeighbours; ++f)
	{
		fn[f].resize(W, H, 1);
		fn[f].copyDataFrom(nbNs + f * npix);
		for(int k = 0; k < nbOfLayers; ++k)
		{
			const size_t i = size_t(f) * nbOfLayers + k;
			fc[i].resize(W, H, 3); fv[i].resize(W, H, 6);
			fc[i].copyDataFrom(nbCols + i * npix * 3); fv[i].copyDataFrom(nbCovs + i * npix * 6);
		}
		DenoiserInputs frame;
		frame.m_pColors = &fc[size_t(f) * nbOfLayers]; frame.m_pNbOfSamples = &fn[f]; frame.m_pHistograms = nullptr; frame.m_pSampleCovariances = &fv[size_t(f) * nbOfLayers];
		if(f < nbOfPlainNeighbours)
		{
			frame.m_pHistograms = &ones;
			pSettings->addNeighbourFrame(frame);
		}
		else
			pSettings->addNeighbourFrameMoments(frame);
		const int given = nbOfLayers - (f == nbOfNeighbours - 1 ? dropLayers : 0);
		for(int k = 1; k < given; ++k)
			pSettings->addNeighbourFrameLayer(size_t(f), &fc[size_t(f) * nbOfLayers + k], &fv[size_t(f) * nbOfLayers + k]);
		if(motions && hasMotion && hasMotion[f])
		{
			mv[f].resize(W, H, 2);
			mv[f].copyDataFrom(motions + f * npix * 2);
			pSettings->setNeighbourMotion(size_t(f), &mv[f]);
		}
		if(features)
		{
			const size_t n = npix * nbOfChannels;
			nf[f].resize(W, H, nbOfChannels); nf[f].copyDataFrom(nbFeatures + f * n);
			if(nbVariances) { nv[f].resize(W, H, nbOfChannels); nv[f].copyDataFrom(nbVariances + f * n); }
			pSettings->setNeighbourGuideFeatures(size_t(f), &nf[f], nbVariances ? &nv[f] : nullptr);
		}
	}
	if(devices && nbOfDevices > 0)
		pSettings->setDevices(std::vector<int>(devices, devices + nbOfDevices));
	d->setInputs(in);
	d->setOutputs(out);
	d->setParameters(p);
	const bool ok = d->denoise();
	if(ok)
		for(int k = 0; k < nbOfLayers; ++k)
			o[k].copyDataTo(outs + k * npix * 3);
	return ok ? 1 : 0;
}

/// ONE MultiscaleDenoiser (or Denoiser), denoise() called twice with -r 0 and the given m_nbOfCores: the written-back core count must not
/// change what the second call does (returns 0 on failure, else 1; nbOfCoresAfter[2] = the field after each call)
int bcdcore_denoise_reuse(const float* col, const float* ns, const float* hist, const float* cov, int W, int H, int D, int nscales, int b,
		int nbOfCores, float* out1, float* out2, int* nbOfCoresAfter)
{
	Deepimf cImg(W, H, 3), nImg(W, H, 1), hImg(W, H, D), vImg(W, H, 6), oImg(W, H, 3);
	cImg.copyDataFrom(col); nImg.copyDataFrom(ns); hImg.copyDataFrom(hist); vImg.copyDataFrom(cov);
	DenoiserInputs in;
	in.m_pColors = &cImg; in.m_pNbOfSamples = &nImg; in.m_pHistograms = &hImg; in.m_pSampleCovariances = &vImg;
	DenoiserOutputs o;
	o.m_pDenoisedColors = &oImg;
	DenoiserParameters p;
	p.m_searchWindowRadius = b;
	p.m_useRandomPixelOrder = false;
	p.m_nbOfCores = nbOfCores;
	std::unique_ptr<IDenoiser> d;
	if(nscales > 1) d.reset(new MultiscaleDenoiser(nscales));
	else d.reset(new Denoiser());
	d->setInputs(in);
	d->setOutputs(o);
	d->setParameters(p);
	float* outs[2] = { out1, out2 };
	for(int i = 0; i < 2; ++i)
	{
		oImg = cImg; // (the multiscale path wants the output pre-sized like the input)
		if(!d->denoise())
			return 0;
		oImg.copyDataTo(outs[i]);
		nbOfCoresAfter[i] = d->getParameters().m_nbOfCores;
	}
	return 1;
}

int bcdcore_spike_filter(float* col, float* ns, float* hist, float* cov, int W, int H, int D, float factor)
{
	Deepimf c(W, H, 3), n(W, H, 1), h(W, H, D), v(W, H, 6);
	c.copyDataFrom(col); n.copyDataFrom(ns); h.copyDataFrom(hist); v.copyDataFrom(cov);
	SpikeRemovalFilter::filter(c, n, h, v, factor);
	c.copyDataTo(col); n.copyDataTo(ns); h.copyDataTo(hist); v.copyDataTo(cov);
	return 0;
}

// the host loops of the prefilter on their own (what filter() runs without a usable device): tests pin them against the reference's fixture on any box
int bcdcore_spike_filter_host(float* col, float* ns, float* hist, float* cov, int W, int H, int D, float factor)
{
	Deepimf c(W, H, 3), n(W, H, 1), h(W, H, D), v(W, H, 6);
	c.copyDataFrom(col); n.copyDataFrom(ns); h.copyDataFrom(hist); v.copyDataFrom(cov);
	SpikeRemovalFilter::filterOnHost(c, n, h, v, factor);
	c.copyDataTo(col); n.copyDataTo(ns); h.copyDataTo(hist); v.copyDataTo(cov);
	return 0;
}

int bcdcore_merge_hist_ns(const float* hist, const float* ns, int W, int H, int D, float* out)
{
	Deepimf h(W, H, D), n(W, H, 1);
	h.copyDataFrom(hist); n.copyDataFrom(ns);
	Utils::mergeHistogramAndNbOfSamples(h, n).copyDataTo(out);
	return 0;
}

int bcdcore_split_hist_ns(const float* in, int W, int H, int Dp1, float* hist, float* ns)
{
	Deepimf m(W, H, Dp1), h, n;
	m.copyDataFrom(in);
	if(!Utils::separateNbOfSamplesFromHistogram(h, n, m)) return -1;
	h.copyDataTo(hist); n.copyDataTo(ns);
	return 0;
}

} // extern "C"

// ---- EXR (ImageIO) ------------------------------------------------------------------------------------------
#include "ImageIO.h"

extern "C" {

int bcdcore_write_exr(const char* path, const float* data, int W, int H, int D, int multiChannels)
{
	Deepimf img(W, H, D);
	img.copyDataFrom(data);
	return (multiChannels ? ImageIO::writeMultiChannelsEXR(img, path) : ImageIO::writeEXR(img, path)) ? 0 : -1;
}

// two-call protocol: out == nullptr -> only the dimensions are returned
int bcdcore_read_exr(const char* path, int multiChannels, int* W, int* H, int* D, float* out, long long capacity)
{
	Deepimf img;
	if(!(multiChannels ? ImageIO::loadMultiChannelsEXR(img, path) : ImageIO::loadEXR(img, path))) return -1;
	*W = img.getWidth(); *H = img.getHeight(); *D = img.getDepth();
	if(out)
	{
		if(capacity < (long long)img.getSize()) return -2;
		img.copyDataTo(out);
	}
	return 0;
}

const char* bcdcore_exr_last_error() { return ImageIO::lastError().c_str(); }

} // extern "C"

// ---- .bcd.json presets (ParametersIO) ----------------------------------------------------------------------------
#include "ParametersIO.h"

extern "C" {

// round trip helper for the tests: loads `in` over the defaults, writes everything to `out`, returns a few fields
int bcdcore_presets_roundtrip(const char* in, const char* out, int* nbOfScales, float* tau, int* b, int* randomOrder, float* m, float* minEig,
		int* spike, float* spikeFactor, char* colorPath, int colorPathCapacity)
{
	PipelineParameters p;
	if(!ParametersIO::load(p, in)) return -1;
	if(out && !ParametersIO::write(p, out)) return -2;
	const DenoiserParameters& d = p.m_denoiserParameters.m_monoscaleParameters;
	*nbOfScales = p.m_denoiserParameters.m_nbOfScales; *tau = d.m_histogramDistanceThreshold; *b = d.m_searchWindowRadius;
	*randomOrder = d.m_useRandomPixelOrder ? 1 : 0; *m = d.m_markedPixelsSkippingProbability; *minEig = d.m_minEigenValue;
	*spike = p.m_prefilteringParameters.m_performSpikeRemoval ? 1 : 0; *spikeFactor = p.m_prefilteringParameters.m_spikeRemovalThresholdStDevFactor;
	snprintf(colorPath, size_t(colorPathCapacity), "%s", p.m_inputFileNames.m_colors.c_str());
	return 0;
}

} // extern "C"
