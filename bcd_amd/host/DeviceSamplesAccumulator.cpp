// DeviceSamplesAccumulator.cpp -- bcd::SamplesAccumulator with its running sums in HBM (bcd_hip_accum_*, k_accumulate.hip).
// addSample appends to a pinned host batch; a full batch (or a snapshot) copies it to the device and applies it through the
// scattered add, which keeps every pixel's samples in call order.  While the device works on one batch the next one fills.
// splatSample does the same with continuous positions through the splatted add; a batch holds calls of one kind only.
// Layers' colours and feature channels ride in pinned arrays of their own beside the batch.
#include "DeviceSamplesAccumulator.h"
#include "bcd_hip.h"

#include <hip/hip_runtime_api.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstring>
#include <utility>

namespace bcd
{

	DeviceSamplesAccumulator::DeviceSamplesAccumulator(int i_width, int i_height, const HistogramParameters& i_rHistogramParameters, int i_device) :
			DeviceSamplesAccumulator(i_width, i_height, i_rHistogramParameters, 0, i_device)
	{
	}

	DeviceSamplesAccumulator::DeviceSamplesAccumulator(int i_width, int i_height, const HistogramParameters& i_rHistogramParameters, int i_nbOfLayers,
			int i_device) :
			m_width(i_width), m_height(i_height), m_nbOfBins(i_rHistogramParameters.m_nbOfBins), m_nbOfLayers(i_nbOfLayers)
	{
		setUp(i_rHistogramParameters, i_device);
	}

	DeviceSamplesAccumulator::DeviceSamplesAccumulator(int i_width, int i_height, const HistogramParameters& i_rHistogramParameters, int i_nbOfLayers,
			int i_nbOfFeatures, int i_device) :
			m_width(i_width), m_height(i_height), m_nbOfBins(i_rHistogramParameters.m_nbOfBins), m_nbOfLayers(i_nbOfLayers), m_nbOfFeatures(i_nbOfFeatures)
	{
		if(i_nbOfFeatures < 1 || i_nbOfFeatures > BCD_HIP_ACCUM_MAX_FEATURES)
		{
			m_error = "the number of feature channels must be in [1, 8]";
			m_nbOfFeatures = 0;
			return;
		}
		setUp(i_rHistogramParameters, i_device);
	}

	void DeviceSamplesAccumulator::setUp(const HistogramParameters& i_rHistogramParameters, int i_device)
	{
		const int i_width = m_width, i_height = m_height;
		if(m_nbOfLayers < 0 || m_nbOfLayers > BCD_HIP_ACCUM_MAX_LAYERS)
		{
			m_error = "the number of layers must be in [0, 15]";
			m_nbOfLayers = 0;
			return;
		}
		int prev = -1;
		(void)hipGetDevice(&prev);
		hipStream_t stream = nullptr;
		if(hipSetDevice(i_device) != hipSuccess || hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess)
		{
			m_error = "no usable HIP device";
			if(prev >= 0) (void)hipSetDevice(prev);
			return;
		}
		m_stream = stream;
		hipEvent_t ev = nullptr;
		const size_t batchBytes = size_t(s_batchCapacity) * (sizeof(int32_t) + 4 * sizeof(float));
		const size_t statsBytes = size_t(i_width) * size_t(i_height) * (10 + 3 * size_t(m_nbOfBins)) * sizeof(float);
		const size_t layerBatchBytes = size_t(m_nbOfLayers) * size_t(s_batchCapacity) * 3 * sizeof(float);
		const size_t layerStatsBytes = size_t(m_nbOfLayers) * size_t(i_width) * size_t(i_height) * 9 * sizeof(float);
		const size_t featureBatchBytes = size_t(m_nbOfFeatures) * size_t(s_batchCapacity) * sizeof(float);
		const size_t featureStatsBytes = size_t(m_nbOfFeatures) * size_t(i_width) * size_t(i_height) * 2 * sizeof(float);
		if(hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess
				|| hipHostMalloc((void**)&m_pHostPixel, size_t(s_batchCapacity) * sizeof(int32_t), hipHostMallocDefault) != hipSuccess
				|| hipHostMalloc((void**)&m_pHostRgbw, size_t(s_batchCapacity) * 4 * sizeof(float), hipHostMallocDefault) != hipSuccess
				|| hipMalloc(&m_pDeviceBatch, batchBytes) != hipSuccess || hipMalloc(&m_pDeviceStats, statsBytes) != hipSuccess
				|| (m_nbOfLayers > 0 && (hipHostMalloc((void**)&m_pHostLayerRgb, layerBatchBytes, hipHostMallocDefault) != hipSuccess
						|| hipMalloc(&m_pDeviceLayerRgb, layerBatchBytes) != hipSuccess || hipMalloc(&m_pDeviceLayerStats, layerStatsBytes) != hipSuccess))
				|| (m_nbOfFeatures > 0 && (hipHostMalloc((void**)&m_pHostFeatures, featureBatchBytes, hipHostMallocDefault) != hipSuccess
						|| hipMalloc(&m_pDeviceFeatures, featureBatchBytes) != hipSuccess || hipMalloc(&m_pDeviceFeatureStats, featureStatsBytes) != hipSuccess)))
		{
			m_batchCopied = ev;
			m_error = "out of device or pinned host memory";
			if(prev >= 0) (void)hipSetDevice(prev);
			return;
		}
		m_batchCopied = ev;
		if(bcd_hip_ctx_create(&m_pContext, i_device, m_stream) != BCD_HIP_OK)
			m_error = "bcd_hip_ctx_create failed";
		else if((m_nbOfFeatures > 0 ? bcd_hip_accum_create_features(m_pContext, i_width, i_height, m_nbOfBins, i_rHistogramParameters.m_gamma,
						i_rHistogramParameters.m_maxValue, s_batchCapacity, m_nbOfLayers, m_nbOfFeatures, &m_pAccum)
				: m_nbOfLayers > 0 ? bcd_hip_accum_create_layers(m_pContext, i_width, i_height, m_nbOfBins, i_rHistogramParameters.m_gamma,
						i_rHistogramParameters.m_maxValue, s_batchCapacity, m_nbOfLayers, &m_pAccum)
				: bcd_hip_accum_create(m_pContext, i_width, i_height, m_nbOfBins, i_rHistogramParameters.m_gamma, i_rHistogramParameters.m_maxValue,
						s_batchCapacity, &m_pAccum)) != BCD_HIP_OK)
		{
			m_error = bcd_hip_last_error(m_pContext);
			m_pAccum = nullptr;
		}
		if(prev >= 0) (void)hipSetDevice(prev);
	}

	DeviceSamplesAccumulator::~DeviceSamplesAccumulator()
	{
		if(m_stream) (void)hipStreamSynchronize((hipStream_t)m_stream);
		bcd_hip_accum_destroy(m_pAccum);
		bcd_hip_ctx_destroy(m_pContext);
		if(m_pDeviceBatch) (void)hipFree(m_pDeviceBatch);
		if(m_pDeviceStats) (void)hipFree(m_pDeviceStats);
		if(m_pDevicePlan) (void)hipFree(m_pDevicePlan);
		if(m_pDeviceLayerRgb) (void)hipFree(m_pDeviceLayerRgb);
		if(m_pDeviceLayerStats) (void)hipFree(m_pDeviceLayerStats);
		if(m_pHostLayerRgb) (void)hipHostFree(m_pHostLayerRgb);
		if(m_pDeviceFeatures) (void)hipFree(m_pDeviceFeatures);
		if(m_pDeviceFeatureStats) (void)hipFree(m_pDeviceFeatureStats);
		if(m_pHostFeatures) (void)hipHostFree(m_pHostFeatures);
		if(m_pHostPixel) (void)hipHostFree(m_pHostPixel);
		if(m_pHostRgbw) (void)hipHostFree(m_pHostRgbw);
		if(m_pHostXy) (void)hipHostFree(m_pHostXy);
		if(m_pDeviceXy) (void)hipFree(m_pDeviceXy);
		if(m_batchCopied) (void)hipEventDestroy((hipEvent_t)m_batchCopied);
		if(m_stream) (void)hipStreamDestroy((hipStream_t)m_stream);
	}

	void DeviceSamplesAccumulator::fail(const char* i_pWhat) const
	{
		m_error = std::string(i_pWhat) + ": " + (m_pContext ? bcd_hip_last_error(m_pContext) : "no context");
	}

	bool DeviceSamplesAccumulator::refusedForFeatures(const char* i_pCall, bool i_withFeatures, const float* i_pFeatures, const float* const* i_ppLayerRgb) const
	{
		const char* why = nullptr;
		if(!i_withFeatures)
			why = m_nbOfFeatures > 0 ? ": an accumulator with feature channels takes the batch form with the samples' features" : nullptr;
		else if(m_nbOfFeatures == 0) why = ": the accumulator has no feature channels";
		else if(!i_pFeatures) why = ": null features";
		else if((i_ppLayerRgb != nullptr) != (m_nbOfLayers > 0)) why = m_nbOfLayers > 0 ? ": null layer colours" : ": layer colours on an accumulator without layers";
		if(why) m_error = std::string(i_pCall) + why;
		return why != nullptr;
	}

	void DeviceSamplesAccumulator::addSample(int i_line, int i_column, float i_sampleR, float i_sampleG, float i_sampleB, float i_weight)
	{
		if(refusedForFeatures("addSample", false, nullptr, nullptr) || !isValid())
			return;
		if(m_nbOfLayers > 0)
		{
			m_error = "addSample: an accumulator with layers takes addSamples with the layers' colours";
			return;
		}
		if(!beginAppend(false))
			return;
		const int64_t i = m_pending++;
		m_pHostPixel[i] = (i_line < 0 || i_line >= m_height || i_column < 0 || i_column >= m_width) ? -1 : i_line * m_width + i_column;
		float* rgb = m_pHostRgbw + 3 * i;
		rgb[0] = i_sampleR; rgb[1] = i_sampleG; rgb[2] = i_sampleB;
		m_pHostRgbw[3 * s_batchCapacity + i] = i_weight;
		if(m_pending == s_batchCapacity)
			flush();
	}

	void DeviceSamplesAccumulator::addSamples(const int32_t* i_pPixelIndices, const float* i_pRgb, const float* i_pWeights, int64_t i_nbOfSamples)
	{
		if(refusedForFeatures("addSamples", false, nullptr, nullptr) || !isValid())
			return;
		if(m_nbOfLayers > 0)
		{
			m_error = "addSamples: an accumulator with layers takes the layers' colours too";
			return;
		}
		appendBatch(false, i_pPixelIndices, i_pRgb, nullptr, nullptr, i_pWeights, i_nbOfSamples);
	}

	void DeviceSamplesAccumulator::addSamples(const int32_t* i_pPixelIndices, const float* i_pRgb, const float* const* i_ppLayerRgb, const float* i_pWeights,
			int64_t i_nbOfSamples)
	{
		if(refusedForFeatures("addSamples", false, nullptr, nullptr) || !isValid())
			return;
		if(m_nbOfLayers == 0 || !i_ppLayerRgb)
		{
			m_error = m_nbOfLayers == 0 ? "addSamples: the accumulator has no layers" : "addSamples: null layer colours";
			return;
		}
		appendBatch(false, i_pPixelIndices, i_pRgb, i_ppLayerRgb, nullptr, i_pWeights, i_nbOfSamples);
	}

	void DeviceSamplesAccumulator::addSamples(const int32_t* i_pPixelIndices, const float* i_pRgb, const float* const* i_ppLayerRgb, const float* i_pFeatures,
			const float* i_pWeights, int64_t i_nbOfSamples)
	{
		if(refusedForFeatures("addSamples", true, i_pFeatures, i_ppLayerRgb) || !isValid())
			return;
		appendBatch(false, i_pPixelIndices, i_pRgb, i_ppLayerRgb, i_pFeatures, i_pWeights, i_nbOfSamples);
	}

	// n samples into the pending batch (i_pKeys: pixel indices, or positions for splats), flushed whenever it is full
	void DeviceSamplesAccumulator::appendBatch(bool i_splat, const void* i_pKeys, const float* i_pRgb, const float* const* i_ppLayerRgb,
			const float* i_pFeatures, const float* i_pWeights, int64_t i_nbOfSamples)
	{
		for(int l = 0; i_ppLayerRgb && l < m_nbOfLayers; ++l)
			if(!i_ppLayerRgb[l])
			{
				m_error = "null layer colours";
				return;
			}
		for(int64_t done = 0; done < i_nbOfSamples; )
		{
			if(!beginAppend(i_splat))
				return;
			const int64_t n = std::min(s_batchCapacity - m_pending, i_nbOfSamples - done);
			if(i_splat) std::memcpy(m_pHostXy + 2 * m_pending, (const float*)i_pKeys + 2 * done, size_t(n) * 2 * sizeof(float));
			else std::memcpy(m_pHostPixel + m_pending, (const int32_t*)i_pKeys + done, size_t(n) * sizeof(int32_t));
			std::memcpy(m_pHostRgbw + 3 * m_pending, i_pRgb + 3 * done, size_t(n) * 3 * sizeof(float));
			for(int l = 0; i_ppLayerRgb && l < m_nbOfLayers; ++l)
				std::memcpy(m_pHostLayerRgb + 3 * (size_t(l) * s_batchCapacity + m_pending), i_ppLayerRgb[l] + 3 * done, size_t(n) * 3 * sizeof(float));
			if(i_pFeatures)
				std::memcpy(m_pHostFeatures + size_t(m_nbOfFeatures) * m_pending, i_pFeatures + size_t(m_nbOfFeatures) * done, size_t(n) * m_nbOfFeatures * sizeof(float));
			float* w = m_pHostRgbw + 3 * s_batchCapacity + m_pending;
			if(i_pWeights) std::memcpy(w, i_pWeights + done, size_t(n) * sizeof(float));
			else std::fill(w, w + n, 1.f);
			m_pending += n;
			done += n;
			if(m_pending == s_batchCapacity)
				flush();
		}
	}

	bool DeviceSamplesAccumulator::beginAppend(bool i_splat)
	{
		if(m_pending > 0 && m_pendingSplats != i_splat && !flush()) // the kind changes: the pending batch goes first, so that pixels see call order
			return false;
		if(m_pending == 0)
		{
			if(m_copyInFlight)
			{	// the previous batch is still being copied out of the pinned buffers
				(void)hipEventSynchronize((hipEvent_t)m_batchCopied);
				m_copyInFlight = false;
			}
			m_pendingSplats = i_splat;
		}
		if(i_splat && !m_pHostXy)
		{
			if(hipHostMalloc((void**)&m_pHostXy, size_t(s_batchCapacity) * 2 * sizeof(float), hipHostMallocDefault) != hipSuccess
					|| hipMalloc(&m_pDeviceXy, size_t(s_batchCapacity) * 2 * sizeof(float)) != hipSuccess)
			{
				m_error = "out of device or pinned host memory for the positions";
				return false;
			}
		}
		return true;
	}

	bool DeviceSamplesAccumulator::setFilter(float i_radiusX, float i_radiusY, int i_tableSize, const float* i_pTable)
	{
		if(!isValid() || !flush())
			return false;
		if(bcd_hip_accum_set_filter(m_pAccum, i_radiusX, i_radiusY, i_tableSize, i_pTable) != BCD_HIP_OK)
		{
			fail("bcd_hip_accum_set_filter");
			return false;
		}
		m_hasFilter = i_pTable != nullptr;
		return true;
	}

	bool DeviceSamplesAccumulator::setFilter(int i_kind, float i_radiusX, float i_radiusY, float i_param, int i_tableSize)
	{
		std::vector<float> table(i_tableSize >= 1 && i_tableSize <= 64 ? size_t(i_tableSize) * i_tableSize : 0);
		if(table.empty() || bcd_hip_filter_table(i_kind, i_radiusX, i_radiusY, i_param, i_tableSize, table.data()) != BCD_HIP_OK)
		{
			m_error = "setFilter: invalid filter kind, radii, parameter or table size";
			return false;
		}
		return setFilter(i_radiusX, i_radiusY, i_tableSize, table.data());
	}

	void DeviceSamplesAccumulator::splatSample(float i_x, float i_y, float i_sampleR, float i_sampleG, float i_sampleB, float i_weight)
	{
		if(refusedForFeatures("splatSample", false, nullptr, nullptr) || !isValid())
			return;
		if(m_nbOfLayers > 0)
		{
			m_error = "splatSample: an accumulator with layers takes splatSamples with the layers' colours";
			return;
		}
		if(!m_hasFilter)
		{
			m_error = "splatSample: no filter (setFilter)";
			return;
		}
		if(!beginAppend(true))
			return;
		const int64_t i = m_pending++;
		m_pHostXy[2 * i] = i_x; m_pHostXy[2 * i + 1] = i_y;
		float* rgb = m_pHostRgbw + 3 * i;
		rgb[0] = i_sampleR; rgb[1] = i_sampleG; rgb[2] = i_sampleB;
		m_pHostRgbw[3 * s_batchCapacity + i] = i_weight;
		if(m_pending == s_batchCapacity)
			flush();
	}

	void DeviceSamplesAccumulator::splatSamples(const float* i_pPositions, const float* i_pRgb, const float* i_pWeights, int64_t i_nbOfSamples)
	{
		if(!isValid())
			return;
		if(!m_hasFilter)
		{
			m_error = "splatSamples: no filter (setFilter)";
			return;
		}
		if(refusedForFeatures("splatSamples", false, nullptr, nullptr))
			return;
		if(m_nbOfLayers > 0)
		{
			m_error = "splatSamples: an accumulator with layers takes the layers' colours too";
			return;
		}
		appendBatch(true, i_pPositions, i_pRgb, nullptr, nullptr, i_pWeights, i_nbOfSamples);
	}

	void DeviceSamplesAccumulator::splatSamples(const float* i_pPositions, const float* i_pRgb, const float* const* i_ppLayerRgb, const float* i_pWeights,
			int64_t i_nbOfSamples)
	{
		if(!isValid())
			return;
		if(!m_hasFilter)
		{
			m_error = "splatSamples: no filter (setFilter)";
			return;
		}
		if(refusedForFeatures("splatSamples", false, nullptr, nullptr))
			return;
		if(m_nbOfLayers == 0 || !i_ppLayerRgb)
		{
			m_error = m_nbOfLayers == 0 ? "splatSamples: the accumulator has no layers" : "splatSamples: null layer colours";
			return;
		}
		appendBatch(true, i_pPositions, i_pRgb, i_ppLayerRgb, nullptr, i_pWeights, i_nbOfSamples);
	}

	void DeviceSamplesAccumulator::splatSamples(const float* i_pPositions, const float* i_pRgb, const float* const* i_ppLayerRgb, const float* i_pFeatures,
			const float* i_pWeights, int64_t i_nbOfSamples)
	{
		if(refusedForFeatures("splatSamples", true, i_pFeatures, i_ppLayerRgb) || !isValid())
			return;
		if(!m_hasFilter)
		{
			m_error = "splatSamples: no filter (setFilter)";
			return;
		}
		appendBatch(true, i_pPositions, i_pRgb, i_ppLayerRgb, i_pFeatures, i_pWeights, i_nbOfSamples);
	}

	bool DeviceSamplesAccumulator::flush() const
	{
		if(!isValid())
			return false;
		if(m_pending == 0)
			return true;
		const int64_t n = m_pending, cap = s_batchCapacity;
		hipStream_t st = (hipStream_t)m_stream;
		int32_t* dPix = (int32_t*)m_pDeviceBatch;
		float* dRgb = (float*)(dPix + cap);
		float* dW = dRgb + 3 * cap;
		const void* hostKeys = m_pendingSplats ? (const void*)m_pHostXy : (const void*)m_pHostPixel;
		void* deviceKeys = m_pendingSplats ? m_pDeviceXy : (void*)dPix;
		const float* dLayers[BCD_HIP_ACCUM_MAX_LAYERS] = { nullptr };
		bool ok = hipMemcpyAsync(deviceKeys, hostKeys, size_t(n) * (m_pendingSplats ? 2 * sizeof(float) : sizeof(int32_t)), hipMemcpyHostToDevice, st) == hipSuccess
				&& hipMemcpyAsync(dRgb, m_pHostRgbw, size_t(n) * 3 * sizeof(float), hipMemcpyHostToDevice, st) == hipSuccess
				&& hipMemcpyAsync(dW, m_pHostRgbw + 3 * cap, size_t(n) * sizeof(float), hipMemcpyHostToDevice, st) == hipSuccess;
		for(int l = 0; ok && l < m_nbOfLayers; ++l)
		{	// the layers' colours leave their pinned buffer ahead of the event too
			float* d = (float*)m_pDeviceLayerRgb + 3 * size_t(l) * cap;
			dLayers[l] = d;
			ok = hipMemcpyAsync(d, m_pHostLayerRgb + 3 * size_t(l) * cap, size_t(n) * 3 * sizeof(float), hipMemcpyHostToDevice, st) == hipSuccess;
		}
		if(ok && m_nbOfFeatures > 0) // (and the feature channels)
			ok = hipMemcpyAsync(m_pDeviceFeatures, m_pHostFeatures, size_t(n) * m_nbOfFeatures * sizeof(float), hipMemcpyHostToDevice, st) == hipSuccess;
		if(!ok || hipEventRecord((hipEvent_t)m_batchCopied, st) != hipSuccess)
		{
			m_error = "batch upload failed";
			return false;
		}
		m_copyInFlight = true;
		m_pending = 0;
		if(m_nbOfFeatures > 0)
		{
			const float* const* layers = m_nbOfLayers > 0 ? dLayers : nullptr;
			const int rc = m_pendingSplats ? bcd_hip_accum_add_splatted_features(m_pAccum, (const float*)m_pDeviceXy, dRgb, dW, n, layers, (const float*)m_pDeviceFeatures)
					: bcd_hip_accum_add_scattered_features(m_pAccum, dPix, dRgb, dW, n, layers, (const float*)m_pDeviceFeatures);
			if(rc != BCD_HIP_OK)
			{
				fail(m_pendingSplats ? "bcd_hip_accum_add_splatted_features" : "bcd_hip_accum_add_scattered_features");
				return false;
			}
			return true;
		}
		if(m_nbOfLayers > 0)
		{
			const int rc = m_pendingSplats ? bcd_hip_accum_add_splatted_layers(m_pAccum, (const float*)m_pDeviceXy, dRgb, dW, n, dLayers)
					: bcd_hip_accum_add_scattered_layers(m_pAccum, dPix, dRgb, dW, n, dLayers);
			if(rc != BCD_HIP_OK)
			{
				fail(m_pendingSplats ? "bcd_hip_accum_add_splatted_layers" : "bcd_hip_accum_add_scattered_layers");
				return false;
			}
			return true;
		}
		if(m_pendingSplats)
		{
			if(bcd_hip_accum_add_splatted(m_pAccum, (const float*)m_pDeviceXy, dRgb, dW, n) != BCD_HIP_OK)
			{
				fail("bcd_hip_accum_add_splatted");
				return false;
			}
			return true;
		}
		if(bcd_hip_accum_add_scattered(m_pAccum, dPix, dRgb, dW, n) != BCD_HIP_OK)
		{
			fail("bcd_hip_accum_add_scattered");
			return false;
		}
		return true;
	}

	DeviceSamplesAccumulator::DeviceStatistics DeviceSamplesAccumulator::computeDeviceStatistics() const
	{
		DeviceStatistics s;
		if(!isValid())
			return s;
		flush();
		const size_t n = size_t(m_width) * size_t(m_height);
		float* p = (float*)m_pDeviceStats;
		s.m_pContext = m_pContext;
		s.m_pNbOfSamples = p;
		s.m_pMean = p + n;
		s.m_pCovariances = p + 4 * n;
		s.m_pHistograms = p + 10 * n;
		s.m_width = m_width; s.m_height = m_height; s.m_depth = 3 * m_nbOfBins;
		if(bcd_hip_accum_statistics(m_pAccum, p, p + n, p + 4 * n, p + 10 * n) != BCD_HIP_OK)
		{
			fail("bcd_hip_accum_statistics");
			return DeviceStatistics();
		}
		return s;
	}

	SamplesStatisticsImages DeviceSamplesAccumulator::getSamplesStatistics() const
	{
		SamplesStatisticsImages out(m_width, m_height, m_nbOfBins);
		const DeviceStatistics d = computeDeviceStatistics();
		if(!d.m_pNbOfSamples)
			return out;
		hipStream_t st = (hipStream_t)m_stream;
		const std::pair<DeepImage<float>*, const float*> parts[4] = { { &out.m_nbOfSamplesImage, d.m_pNbOfSamples }, { &out.m_meanImage, d.m_pMean },
				{ &out.m_covarImage, d.m_pCovariances }, { &out.m_histoImage, d.m_pHistograms } };
		for(const auto& pr : parts)
			if(hipMemcpyAsync(pr.first->getDataPtr(), pr.second, pr.first->getDataPtr() ? size_t(m_width) * m_height * pr.first->getDepth() * sizeof(float) : 0,
					hipMemcpyDeviceToHost, st) != hipSuccess)
				m_error = "statistics download failed";
		if(hipStreamSynchronize(st) != hipSuccess)
			m_error = "statistics download failed";
		return out;
	}

	std::vector<DeviceSamplesAccumulator::DeviceLayerStatistics> DeviceSamplesAccumulator::computeDeviceLayerStatistics() const
	{
		std::vector<DeviceLayerStatistics> out;
		if(!isValid() || m_nbOfLayers == 0)
			return out;
		flush();
		const size_t n = size_t(m_width) * size_t(m_height);
		float* means[BCD_HIP_ACCUM_MAX_LAYERS];
		float* covs[BCD_HIP_ACCUM_MAX_LAYERS];
		for(int l = 0; l < m_nbOfLayers; ++l)
		{
			means[l] = (float*)m_pDeviceLayerStats + size_t(l) * 9 * n;
			covs[l] = means[l] + 3 * n;
		}
		if(bcd_hip_accum_layer_statistics(m_pAccum, means, covs) != BCD_HIP_OK)
		{
			fail("bcd_hip_accum_layer_statistics");
			return out;
		}
		out.resize(size_t(m_nbOfLayers));
		for(int l = 0; l < m_nbOfLayers; ++l)
		{
			out[size_t(l)].m_pMean = means[l];
			out[size_t(l)].m_pCovariances = covs[l];
		}
		return out;
	}

	bool DeviceSamplesAccumulator::getLayerStatistics(int i_layer, Deepimf& o_rMean, Deepimf& o_rCovariances) const
	{
		if(!isValid())
			return false;
		if(i_layer < 0 || i_layer >= m_nbOfLayers)
		{
			m_error = "getLayerStatistics: no such layer";
			return false;
		}
		const std::vector<DeviceLayerStatistics> d = computeDeviceLayerStatistics();
		if(d.empty())
			return false;
		o_rMean.resize(m_width, m_height, 3);
		o_rCovariances.resize(m_width, m_height, 6);
		const size_t n = size_t(m_width) * size_t(m_height);
		hipStream_t st = (hipStream_t)m_stream;
		if(hipMemcpyAsync(o_rMean.getDataPtr(), d[size_t(i_layer)].m_pMean, n * 3 * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess
				|| hipMemcpyAsync(o_rCovariances.getDataPtr(), d[size_t(i_layer)].m_pCovariances, n * 6 * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess
				|| hipStreamSynchronize(st) != hipSuccess)
		{
			m_error = "layer statistics download failed";
			return false;
		}
		return true;
	}

	DeviceSamplesAccumulator::DeviceFeatureStatistics DeviceSamplesAccumulator::computeDeviceFeatureStatistics() const
	{
		DeviceFeatureStatistics s;
		if(!isValid() || m_nbOfFeatures == 0)
			return s;
		flush();
		float* p = (float*)m_pDeviceFeatureStats;
		const size_t n = size_t(m_width) * size_t(m_height) * size_t(m_nbOfFeatures);
		if(bcd_hip_accum_feature_statistics(m_pAccum, p, p + n) != BCD_HIP_OK)
		{
			fail("bcd_hip_accum_feature_statistics");
			return s;
		}
		s.m_pFeatures = p;
		s.m_pVariances = p + n;
		s.m_nbOfChannels = m_nbOfFeatures;
		return s;
	}

	bool DeviceSamplesAccumulator::getFeatureStatistics(Deepimf& o_rMean, Deepimf& o_rVarianceOfMean) const
	{
		if(!isValid())
			return false;
		if(m_nbOfFeatures == 0)
		{
			m_error = "getFeatureStatistics: the accumulator has no feature channels";
			return false;
		}
		const DeviceFeatureStatistics d = computeDeviceFeatureStatistics();
		if(!d.m_pFeatures)
			return false;
		o_rMean.resize(m_width, m_height, m_nbOfFeatures);
		o_rVarianceOfMean.resize(m_width, m_height, m_nbOfFeatures);
		const size_t bytes = size_t(m_width) * size_t(m_height) * size_t(m_nbOfFeatures) * sizeof(float);
		hipStream_t st = (hipStream_t)m_stream;
		if(hipMemcpyAsync(o_rMean.getDataPtr(), d.m_pFeatures, bytes, hipMemcpyDeviceToHost, st) != hipSuccess
				|| hipMemcpyAsync(o_rVarianceOfMean.getDataPtr(), d.m_pVariances, bytes, hipMemcpyDeviceToHost, st) != hipSuccess
				|| hipStreamSynchronize(st) != hipSuccess)
		{
			m_error = "feature statistics download failed";
			return false;
		}
		return true;
	}

	SamplesStatisticsImages DeviceSamplesAccumulator::extractSamplesStatistics()
	{
		SamplesStatisticsImages out = getSamplesStatistics();
		m_isValid = false;
		return out;
	}

	bool DeviceSamplesAccumulator::planSamples(int64_t i_budget, uint64_t i_offset, const PlanParameters& i_rParameters,
			std::vector<int32_t>& o_pixelIndices, PlanSummary* o_pSummary)
	{
		o_pixelIndices.clear();
		if(!isValid())
			return false;
		if(i_budget < 0 || i_budget > INT32_MAX)
		{	// (before the list buffer grows to the budget)
			m_error = "planSamples: the budget must be in [0, 2^31)";
			return false;
		}
		if(!flush()) // this call's own flush; an earlier failure (still in lastError()) does not block the plan
			return false;
		const int64_t capacity = std::max<int64_t>(i_budget, 1);
		if(capacity > m_planCapacity)
		{
			if(m_pDevicePlan && (hipStreamSynchronize((hipStream_t)m_stream) != hipSuccess || hipFree(m_pDevicePlan) != hipSuccess))
			{
				m_error = "plan buffer release failed";
				return false;
			}
			m_pDevicePlan = nullptr;
			m_planCapacity = -1;
			if(hipMalloc(&m_pDevicePlan, sizeof(bcd_hip_plan_summary) + size_t(capacity) * sizeof(int32_t)) != hipSuccess)
			{
				m_pDevicePlan = nullptr;
				m_error = "out of device memory for the plan";
				return false;
			}
			m_planCapacity = capacity;
		}
		bcd_hip_plan_params prm;
		prm.threshold = i_rParameters.m_threshold;
		prm.eps = i_rParameters.m_eps;
		prm.min_samples = i_rParameters.m_minSamples;
		prm.max_per_pixel = i_rParameters.m_maxPerPixel;
		bcd_hip_plan_summary* dSummary = (bcd_hip_plan_summary*)m_pDevicePlan;
		int32_t* dPixels = (int32_t*)(dSummary + 1);
		if(bcd_hip_accum_plan(m_pAccum, &prm, i_budget, i_offset, nullptr, nullptr, dPixels, m_planCapacity, dSummary) != BCD_HIP_OK)
		{
			fail("bcd_hip_accum_plan");
			return false;
		}
		bcd_hip_plan_summary summary;
		hipStream_t st = (hipStream_t)m_stream;
		if(hipMemcpyAsync(&summary, dSummary, sizeof(summary), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
		{
			m_error = "plan download failed";
			return false;
		}
		o_pixelIndices.resize(size_t(summary.planned));
		if(summary.planned > 0 && (hipMemcpyAsync(o_pixelIndices.data(), dPixels, size_t(summary.planned) * sizeof(int32_t), hipMemcpyDeviceToHost, st)
				!= hipSuccess || hipStreamSynchronize(st) != hipSuccess))
		{
			o_pixelIndices.clear();
			m_error = "plan download failed";
			return false;
		}
		if(o_pSummary)
		{
			o_pSummary->m_planned = summary.planned;
			o_pSummary->m_active = summary.active;
			o_pSummary->m_unsampled = summary.unsampled;
			o_pSummary->m_maxError = summary.max_error;
		}
		return true;
	}

	bool DeviceSamplesAccumulator::exportState(std::vector<uint8_t>& o_state) const
	{
		o_state.clear();
		if(!isValid() || !flush())
			return false;
		int64_t bytes = 0;
		if(bcd_hip_accum_state_bytes(m_pAccum, &bytes) != BCD_HIP_OK)
		{
			fail("bcd_hip_accum_state_bytes");
			return false;
		}
		o_state.resize(size_t(bytes));
		if(bcd_hip_accum_export(m_pAccum, o_state.data(), bytes) != BCD_HIP_OK)
		{
			o_state.clear();
			fail("bcd_hip_accum_export");
			return false;
		}
		return true;
	}

	bool DeviceSamplesAccumulator::saveState(const std::string& i_rPath) const
	{
		return toFile(i_rPath, BLOCK_STATE);
	}

	bool DeviceSamplesAccumulator::saveLayers(const std::string& i_rPath) const
	{
		return toFile(i_rPath, BLOCK_LAYERS);
	}

	bool DeviceSamplesAccumulator::loadLayers(const std::string& i_rPath)
	{
		return fromFile(i_rPath, false, BLOCK_LAYERS);
	}

	bool DeviceSamplesAccumulator::mergeLayers(const std::string& i_rPath)
	{
		return fromFile(i_rPath, true, BLOCK_LAYERS);
	}

	bool DeviceSamplesAccumulator::saveFeatures(const std::string& i_rPath) const
	{
		return toFile(i_rPath, BLOCK_FEATURES);
	}

	bool DeviceSamplesAccumulator::loadFeatures(const std::string& i_rPath)
	{
		return fromFile(i_rPath, false, BLOCK_FEATURES);
	}

	bool DeviceSamplesAccumulator::mergeFeatures(const std::string& i_rPath)
	{
		return fromFile(i_rPath, true, BLOCK_FEATURES);
	}

	bool DeviceSamplesAccumulator::toFile(const std::string& i_rPath, Block i_block) const
	{
		if(!isValid() || !flush())
			return false;
		int64_t bytes = 0;
		if((i_block == BLOCK_FEATURES ? bcd_hip_accum_features_state_bytes(m_pAccum, &bytes)
				: i_block == BLOCK_LAYERS ? bcd_hip_accum_layers_state_bytes(m_pAccum, &bytes) : bcd_hip_accum_state_bytes(m_pAccum, &bytes)) != BCD_HIP_OK)
		{
			fail(i_block == BLOCK_FEATURES ? "bcd_hip_accum_features_state_bytes" : i_block == BLOCK_LAYERS ? "bcd_hip_accum_layers_state_bytes" : "bcd_hip_accum_state_bytes");
			return false;
		}
		const int fd = open(i_rPath.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
		if(fd < 0)
		{
			m_error = "saveState: cannot create '" + i_rPath + "': " + std::strerror(errno);
			return false;
		}
		// the blocks are reserved before the mapping is written (a full disk fails here, not with a fault on a page of the mapping)
		const int err = posix_fallocate(fd, 0, off_t(bytes));
		void* p = err == 0 ? mmap(nullptr, size_t(bytes), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0) : MAP_FAILED;
		close(fd);
		if(p == MAP_FAILED)
		{
			m_error = "saveState: cannot write " + std::to_string(bytes) + " bytes to '" + i_rPath + "': " + std::strerror(err ? err : errno);
			unlink(i_rPath.c_str());
			return false;
		}
		const int rc = i_block == BLOCK_FEATURES ? bcd_hip_accum_export_features(m_pAccum, p, bytes)
				: i_block == BLOCK_LAYERS ? bcd_hip_accum_export_layers(m_pAccum, p, bytes) : bcd_hip_accum_export(m_pAccum, p, bytes);
		munmap(p, size_t(bytes));
		if(rc != BCD_HIP_OK)
		{
			fail(i_block == BLOCK_FEATURES ? "bcd_hip_accum_export_features" : i_block == BLOCK_LAYERS ? "bcd_hip_accum_export_layers" : "bcd_hip_accum_export");
			unlink(i_rPath.c_str());
			return false;
		}
		return true;
	}

	bool DeviceSamplesAccumulator::fromFile(const std::string& i_rPath, bool i_merge, Block i_block)
	{
		const char* what = i_block == BLOCK_FEATURES ? (i_merge ? "mergeFeatures" : "loadFeatures")
				: i_block == BLOCK_LAYERS ? (i_merge ? "mergeLayers" : "loadLayers") : (i_merge ? "mergeState" : "loadState");
		if(!isValid() || !flush())
			return false;
		const int fd = open(i_rPath.c_str(), O_RDONLY);
		if(fd < 0)
		{
			m_error = std::string(what) + ": cannot open '" + i_rPath + "': " + std::strerror(errno);
			return false;
		}
		struct stat sb;
		if(fstat(fd, &sb) != 0 || sb.st_size < BCD_HIP_ACCUM_STATE_HEADER_BYTES)
		{
			close(fd);
			m_error = std::string(what) + ": '" + i_rPath + "' is not an accumulator state (shorter than its 64-byte header)";
			return false;
		}
		const size_t bytes = size_t(sb.st_size);
		void* p = mmap(nullptr, bytes, PROT_READ, MAP_PRIVATE, fd, 0);
		close(fd);
		if(p == MAP_FAILED)
		{
			m_error = std::string(what) + ": cannot map '" + i_rPath + "': " + std::strerror(errno);
			return false;
		}
		(void)madvise(p, bytes, MADV_SEQUENTIAL);
		// both calls return once the mapping is no longer needed
		const int rc = i_block == BLOCK_FEATURES
				? (i_merge ? bcd_hip_accum_merge_features_state(m_pAccum, p, int64_t(bytes)) : bcd_hip_accum_import_features(m_pAccum, p, int64_t(bytes)))
				: i_block == BLOCK_LAYERS ? (i_merge ? bcd_hip_accum_merge_layers_state(m_pAccum, p, int64_t(bytes)) : bcd_hip_accum_import_layers(m_pAccum, p, int64_t(bytes)))
				: (i_merge ? bcd_hip_accum_merge_state(m_pAccum, p, int64_t(bytes)) : bcd_hip_accum_import(m_pAccum, p, int64_t(bytes)));
		munmap(p, bytes);
		if(rc != BCD_HIP_OK)
		{
			fail((std::string(what) + " '" + i_rPath + "'").c_str());
			return false;
		}
		return true;
	}

	bool DeviceSamplesAccumulator::loadState(const std::string& i_rPath)
	{
		return fromFile(i_rPath, false);
	}

	bool DeviceSamplesAccumulator::mergeState(const std::string& i_rPath)
	{
		return fromFile(i_rPath, true);
	}

	bool DeviceSamplesAccumulator::merge(const DeviceSamplesAccumulator& i_rOther)
	{
		if(!isValid())
			return false;
		if(!i_rOther.isValid())
		{
			m_error = "merge: the other accumulator is not valid";
			return false;
		}
		if(!flush())
			return false;
		if(!i_rOther.flush())
		{
			m_error = "merge: the other accumulator: " + i_rOther.lastError();
			return false;
		}
		if(bcd_hip_accum_merge(m_pAccum, i_rOther.m_pAccum) != BCD_HIP_OK)
		{
			fail("bcd_hip_accum_merge");
			return false;
		}
		return true;
	}

	void DeviceSamplesAccumulator::reset()
	{
		if(!isValid())
			return;
		m_pending = 0;
		if(bcd_hip_accum_reset(m_pAccum) != BCD_HIP_OK)
			fail("bcd_hip_accum_reset");
	}

	int64_t DeviceSamplesAccumulator::nbOfAccumulatedSamples() const
	{
		flush();
		int64_t added = 0;
		if(m_pAccum && bcd_hip_accum_info(m_pAccum, &added, nullptr) != BCD_HIP_OK)
			fail("bcd_hip_accum_info");
		return added;
	}

	int64_t DeviceSamplesAccumulator::nbOfDroppedSamples() const
	{
		flush();
		int64_t dropped = 0;
		if(m_pAccum && bcd_hip_accum_info(m_pAccum, nullptr, &dropped) != BCD_HIP_OK)
			fail("bcd_hip_accum_info");
		return dropped;
	}

} // namespace bcd
