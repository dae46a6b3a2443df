// DeviceSamplesAccumulator.h -- SamplesAccumulator whose running sums live in HBM (the bcd_hip_accum_* entry points of bcd_hip.h).
// Same public surface as bcd::SamplesAccumulator (SamplesAccumulator.h): addSample buffers on the host in call order and the buffer
// is flushed through the device's scattered add, so every pixel accumulates its samples in call order with the host class's float
// operations (nSamples, mean and covariance bit-identical; histograms to the device powf's round-off).  Snapshots are non-destructive
// and can stay on the device for bcd_hip_denoise.
// Colour layers: an accumulator constructed with a layer count keeps nine more running sums per layer beside the beauty's (the
// bcd_hip_accum_*_layers entry points of bcd_hip.h, which define them exactly).  Such an accumulator is fed through the batch forms of
// addSamples / splatSamples that take the layers' colour arrays; the single-sample addSample / splatSample have no form with layers and
// are refused on it (message in lastError()), as are the batch forms without layers.
// Feature channels: an accumulator constructed with a feature count keeps two more running sums per channel (the bcd_hip_accum_*_features
// entry points of bcd_hip.h, which define them exactly) and snapshots them into the feature and variance images of a bcd_hip_guide.  It is
// fed through the batch forms of addSamples / splatSamples that take the samples' feature channels; every other add is refused on it.
#ifndef DEVICE_SAMPLES_ACCUMULATOR_H
#define DEVICE_SAMPLES_ACCUMULATOR_H

#include "SamplesAccumulator.h"

#include <cstdint>
#include <string>
#include <vector>

struct bcd_hip_ctx;
struct bcd_hip_accum;

namespace bcd
{

	class DeviceSamplesAccumulator
	{
	public:
		/// device statistics images in DeepImage layout, owned by the accumulator and valid until the next snapshot or destruction;
		/// the arguments of bcd_hip_denoise(context, m_pMean, m_pNbOfSamples, m_pHistograms, m_pCovariances, width, height, depth, ...)
		struct DeviceStatistics
		{
			bcd_hip_ctx* m_pContext = nullptr; ///< the context whose stream orders the snapshot
			const float* m_pNbOfSamples = nullptr;
			const float* m_pMean = nullptr;
			const float* m_pCovariances = nullptr;
			const float* m_pHistograms = nullptr;
			int m_width = 0, m_height = 0, m_depth = 0;
		};

		/// adaptive sample planning (bcd_hip_accum_plan in bcd_hip.h, which defines the plan exactly)
		struct PlanParameters
		{
			float m_threshold = 0.f;  ///< pixels whose relative error is at most this get no samples
			float m_eps = 1e-3f;      ///< added to the luminance in the relative error
			float m_minSamples = 2.f; ///< pixels with a smaller weight sum have an infinite error
			int m_maxPerPixel = 16;   ///< cap of the samples one pixel gets in one plan, in [1, 65535]
		};
		struct PlanSummary
		{
			int64_t m_planned = 0;   ///< entries of the pixel list
			int64_t m_active = 0;    ///< pixels with an error above the threshold
			int64_t m_unsampled = 0; ///< active pixels with an infinite error
			float m_maxError = 0.f;  ///< largest finite error of the active pixels
		};

		/// one layer's statistics on the device, owned by the accumulator and valid until the next layer snapshot or destruction: with the
		/// beauty's DeviceStatistics (m_pMean, m_pCovariances) first, the layers of bcd_hip_denoise_layers
		struct DeviceLayerStatistics
		{
			const float* m_pMean = nullptr;
			const float* m_pCovariances = nullptr;
		};

		/// the feature statistics on the device, owned by the accumulator and valid until the next feature snapshot or destruction: the
		/// features and variances of a bcd_hip_guide with nb_channels = m_nbOfChannels, width * height * m_nbOfChannels floats each
		struct DeviceFeatureStatistics
		{
			const float* m_pFeatures = nullptr;  ///< every channel's weighted mean over the pixel's samples
			const float* m_pVariances = nullptr; ///< the variance of that mean
			int m_nbOfChannels = 0;
		};

		DeviceSamplesAccumulator(int i_width, int i_height, const HistogramParameters& i_rHistogramParameters, int i_device = 0);
		/// with i_nbOfLayers extra colour layers, in [1, 15] (otherwise the accumulator is not valid)
		DeviceSamplesAccumulator(int i_width, int i_height, const HistogramParameters& i_rHistogramParameters, int i_nbOfLayers, int i_device);
		/// with i_nbOfLayers extra colour layers, in [0, 15], and i_nbOfFeatures auxiliary feature channels, in [1, 8] (otherwise the
		/// accumulator is not valid)
		DeviceSamplesAccumulator(int i_width, int i_height, const HistogramParameters& i_rHistogramParameters, int i_nbOfLayers, int i_nbOfFeatures,
				int i_device);
		int nbOfLayers() const { return m_nbOfLayers; }
		int nbOfFeatures() const { return m_nbOfFeatures; }
		~DeviceSamplesAccumulator();
		DeviceSamplesAccumulator(const DeviceSamplesAccumulator&) = delete;
		DeviceSamplesAccumulator& operator=(const DeviceSamplesAccumulator&) = delete;

		/// false when the device could not be set up (message in lastError()); every other call is then a no-op
		bool isValid() const { return m_pAccum != nullptr && m_isValid; }
		const std::string& lastError() const { return m_error; }

		void addSample(int i_line, int i_column, float i_sampleR, float i_sampleG, float i_sampleB, float i_weight = 1.f);
		/// n samples from host memory, in order: pixel index line * width + column, rgb [n][3], weights [n] or nullptr (all 1).
		/// Indices outside the frame are skipped (and counted by nbOfDroppedSamples()).
		void addSamples(const int32_t* i_pPixelIndices, const float* i_pRgb, const float* i_pWeights, int64_t i_nbOfSamples);

		/// the same with the layers' colours: i_ppLayerRgb[nbOfLayers()], each [n][3], same pixels, weights and order as the beauty's
		void addSamples(const int32_t* i_pPixelIndices, const float* i_pRgb, const float* const* i_ppLayerRgb, const float* i_pWeights, int64_t i_nbOfSamples);

		/// the same with the samples' feature channels, on an accumulator with features: i_pFeatures [n][nbOfFeatures()]; i_ppLayerRgb is
		/// nullptr exactly when the accumulator has no layers
		void addSamples(const int32_t* i_pPixelIndices, const float* i_pRgb, const float* const* i_ppLayerRgb, const float* i_pFeatures, const float* i_pWeights,
				int64_t i_nbOfSamples);

		/// Pixel reconstruction filter of splatSample / splatSamples (bcd_hip_accum_set_filter in bcd_hip.h, which defines the splat exactly):
		/// radii in (0, 3], a table of i_tableSize x i_tableSize finite values >= 0 (row = y index), i_tableSize in [1, 64]; a null table
		/// removes the filter.  The samples buffered so far are applied first (splats with the previous filter).  false with lastError()
		/// for invalid arguments, the previous filter kept.  The filter is not part of a saved state.
		bool setFilter(float i_radiusX, float i_radiusY, int i_tableSize, const float* i_pTable);
		/// a standard separable filter (bcd_hip_filter_table): i_kind BCD_HIP_FILTER_BOX, _TENT, _GAUSSIAN (i_param = alpha), _BLACKMAN_HARRIS
		bool setFilter(int i_kind, float i_radiusX, float i_radiusY, float i_param = 2.f, int i_tableSize = 16);
		/// a sample at the continuous position (i_x, i_y) -- pixel (column, line) covers [column, column + 1) x [line, line + 1) -- given to
		/// every pixel of its filter footprint with weight i_weight * filter value.  Buffered like addSample; calls of addSample and
		/// splatSample may interleave, every pixel still sees call order.  Without a filter the sample is refused (lastError()).
		void splatSample(float i_x, float i_y, float i_sampleR, float i_sampleG, float i_sampleB, float i_weight = 1.f);
		/// n samples from host memory, in order: positions [n][2] (x, y), rgb [n][3], weights [n] or nullptr (all 1)
		void splatSamples(const float* i_pPositions, const float* i_pRgb, const float* i_pWeights, int64_t i_nbOfSamples);

		/// the same with the layers' colours: i_ppLayerRgb[nbOfLayers()], each [n][3]
		void splatSamples(const float* i_pPositions, const float* i_pRgb, const float* const* i_ppLayerRgb, const float* i_pWeights, int64_t i_nbOfSamples);

		/// the same with the samples' feature channels: i_pFeatures [n][nbOfFeatures()]; i_ppLayerRgb is nullptr exactly without layers
		void splatSamples(const float* i_pPositions, const float* i_pRgb, const float* const* i_ppLayerRgb, const float* i_pFeatures, const float* i_pWeights,
				int64_t i_nbOfSamples);

		/// copy of the statistics accumulated so far (the accumulator goes on)
		SamplesStatisticsImages getSamplesStatistics() const;
		/// moves the statistics out; the accumulator must not be used afterwards
		SamplesStatisticsImages extractSamplesStatistics();
		/// enqueues a snapshot into device buffers owned by the accumulator (no host copy, no synchronisation) and returns them
		DeviceStatistics computeDeviceStatistics() const;

		/// enqueues a snapshot of every layer into device buffers owned by the accumulator (no host copy, no synchronisation); empty on
		/// failure or without layers
		std::vector<DeviceLayerStatistics> computeDeviceLayerStatistics() const;
		/// host copy of layer i_layer's mean (depth 3) and covariance (depth 6) images; synchronises
		bool getLayerStatistics(int i_layer, Deepimf& o_rMean, Deepimf& o_rCovariances) const;

		/// enqueues a snapshot of the feature channels into device buffers owned by the accumulator (no host copy, no synchronisation);
		/// null pointers on failure or without features
		DeviceFeatureStatistics computeDeviceFeatureStatistics() const;
		/// host copy of the feature means and of the variances of those means (depth nbOfFeatures() each); synchronises
		bool getFeatureStatistics(Deepimf& o_rMean, Deepimf& o_rVarianceOfMean) const;

		/// where the next i_budget samples go: o_pixelIndices receives the planned pixel indices (line * width + column) in ascending order,
		/// each pixel repeated as many times as it gets samples.  The samples buffered by addSample are applied first; the statistics are
		/// not changed.  Synchronises.  false (message in lastError()) for invalid parameters or a device error; a failed call does not
		/// affect the next one.
		bool planSamples(int64_t i_budget, uint64_t i_offset, const PlanParameters& i_rParameters, std::vector<int32_t>& o_pixelIndices,
				PlanSummary* o_pSummary = nullptr);

		/// States (bcd_hip_accum_export / _import / _merge_state / _merge in bcd_hip.h, which define the format v1 and the merge).  Each call
		/// applies the samples buffered by addSample first (on both accumulators for merge) and returns false with lastError() on failure;
		/// the accumulator stays usable.  Files are mapped, not read into a second host copy.
		/// the serialised state (header + planes); synchronises
		bool exportState(std::vector<uint8_t>& o_state) const;
		/// the serialised state written to a file (replaced if it exists)
		bool saveState(const std::string& i_rPath) const;
		/// replaces the state and counters with a file's; its frame size, bins, gamma and max value must be this accumulator's
		bool loadState(const std::string& i_rPath);
		/// adds a file's state into this one (one fp32 add per running sum)
		bool mergeState(const std::string& i_rPath);
		/// adds another accumulator's state into this one; the other may live on another device and is not changed
		bool merge(const DeviceSamplesAccumulator& i_rOther);

		/// The layer block (bcd_hip_accum_export_layers / _import_layers / _merge_layers_state in bcd_hip.h): the layers' running sums, a file
		/// of its own beside the state's.  A checkpoint of an accumulator with layers is saveState plus saveLayers.
		bool saveLayers(const std::string& i_rPath) const;
		bool loadLayers(const std::string& i_rPath);
		bool mergeLayers(const std::string& i_rPath);

		/// The feature block (bcd_hip_accum_export_features / _import_features / _merge_features_state in bcd_hip.h): the feature channels'
		/// running sums, a file of its own.  A checkpoint of an accumulator with features is saveState plus saveFeatures (plus saveLayers).
		bool saveFeatures(const std::string& i_rPath) const;
		bool loadFeatures(const std::string& i_rPath);
		bool mergeFeatures(const std::string& i_rPath);

		/// back to an empty accumulator (the frame geometry and the device buffers are kept)
		void reset();
		/// samples accumulated / skipped since construction or the last reset (synchronises)
		int64_t nbOfAccumulatedSamples() const;
		int64_t nbOfDroppedSamples() const;

	private:
		/// applies the pending addSample batch; false (message in lastError()) if this flush failed
		bool flush() const;
		void fail(const char* i_pWhat) const;
		/// loadState / mergeState: the mapped file through bcd_hip_accum_import (merge = false) or _merge_state
		enum Block { BLOCK_STATE = 0, BLOCK_LAYERS = 1, BLOCK_FEATURES = 2 };
		bool fromFile(const std::string& i_rPath, bool i_merge, Block i_block = BLOCK_STATE);
		bool toFile(const std::string& i_rPath, Block i_block) const;
		void appendBatch(bool i_splat, const void* i_pKeys, const float* i_pRgb, const float* const* i_ppLayerRgb, const float* i_pFeatures,
				const float* i_pWeights, int64_t i_nbOfSamples);
		void setUp(const HistogramParameters& i_rHistogramParameters, int i_device);
		/// the refusals of the forms without features on an accumulator with features, and of the batch forms with them elsewhere (decided
		/// from the arguments and the counts alone, before the device is looked at)
		bool refusedForFeatures(const char* i_pCall, bool i_withFeatures, const float* i_pFeatures, const float* const* i_ppLayerRgb) const;

	private:
		int m_width, m_height, m_nbOfBins;
		int m_nbOfLayers = 0;
		float* m_pHostLayerRgb = nullptr;    // the layers' colours of the pending batch [layer][capacity][3] (pinned), and their device copy
		void* m_pDeviceLayerRgb = nullptr;
		void* m_pDeviceLayerStats = nullptr; // per layer mean | cov of computeDeviceLayerStatistics
		int m_nbOfFeatures = 0;
		float* m_pHostFeatures = nullptr;    // the feature channels of the pending batch [capacity][nbOfFeatures] (pinned), and their device copy
		void* m_pDeviceFeatures = nullptr;
		void* m_pDeviceFeatureStats = nullptr; // features | variances of computeDeviceFeatureStatistics
		bcd_hip_ctx* m_pContext = nullptr;
		bcd_hip_accum* m_pAccum = nullptr;
		bool m_isValid = true;
		mutable std::string m_error;
		// host-side batch of addSample calls (pinned), and its device copy
		static const int64_t s_batchCapacity = int64_t(1) << 20;
		mutable int64_t m_pending = 0;
		bool m_pendingSplats = false;   // the pending batch holds splatSample calls (positions in m_pHostXy), not addSample calls
		bool m_hasFilter = false;
		float* m_pHostXy = nullptr;     // positions [capacity][2] (pinned) and their device copy, allocated by the first splat
		void* m_pDeviceXy = nullptr;
		/// the batch buffers of the kind about to be appended to are free: flushes a pending batch of the other kind, waits for the copy
		/// of the previous batch
		bool beginAppend(bool i_splat);
		int32_t* m_pHostPixel = nullptr;
		float* m_pHostRgbw = nullptr; // rgb [capacity][3] then weights [capacity]
		void* m_pDeviceBatch = nullptr;
		void* m_stream = nullptr;        // hipStream_t of the context
		void* m_batchCopied = nullptr;   // hipEvent_t: the pinned batch has reached the device
		mutable bool m_copyInFlight = false;
		void* m_pDeviceStats = nullptr; // ns | mean | cov | hist of computeDeviceStatistics
		void* m_pDevicePlan = nullptr;  // summary (32 bytes) | pixel list of planSamples (grow-only)
		int64_t m_planCapacity = -1;
	};

} // namespace bcd

#endif // DEVICE_SAMPLES_ACCUMULATOR_H
