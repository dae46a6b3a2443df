// Denoiser.cpp -- bcd::Denoiser / bcd::MultiscaleDenoiser of the MI355X build: input validation with the
// reference's messages and return values (src/core/Denoiser.cpp:238-348), then one call into the C ABI
// (include/bcd_hip.h) which runs the whole loop on the device.  No CPU fallback: a missing device is an error.
#include "Denoiser.h"
#include "MultiscaleDenoiser.h"
#include "SpikeRemovalFilter.h"

#include "bcd_hip.h"

#include <functional>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <omp.h>
#include <vector>

using namespace std;

namespace bcd
{

	bool Denoiser::inputsOutputsAreOk()
	{
		const DeepImage<float>* images[4] = { m_inputs.m_pColors, m_inputs.m_pNbOfSamples, m_inputs.m_pHistograms, m_inputs.m_pSampleCovariances };
		const char* names[4] = { "color", "number of samples", "histogram", "covariance" };
		bool ok = true;
		if(m_momentSelection)
			images[2] = images[0] ? images[0] : images[3]; // no histogram image is looked at: its slot repeats another image for the checks below
		for(int i = 0; i < 4; ++i)
			if(!images[i])
			{
				ok = false;
				cerr << "Aborting denoising: nullptr for input " << names[i] << " image" << endl;
			}
		if(!ok)
			return false;
		if(!m_outputs.m_pDenoisedColors)
		{
			cerr << "Aborting denoising: nullptr for output image" << endl;
			return false;
		}
		for(int i = 0; i < 4; ++i)
			if(images[i]->isEmpty())
			{
				ok = false;
				cerr << "Aborting denoising: input " << names[i] << " image is empty" << endl;
			}
		if(!ok)
			return false;
		const int w = images[0]->getWidth(), h = images[0]->getHeight();
		for(int i = 1; i < 4; ++i)
			if(images[i]->getWidth() != w || images[i]->getHeight() != h)
			{
				ok = false;
				cerr << "Aborting denoising: input " << names[i] << " image is " << images[i]->getWidth() << "x" << images[i]->getHeight()
						<< " but input color image is " << w << "x" << h << endl;
			}
		if(!ok)
			return false;
		if(images[0]->getDepth() != 3 || images[1]->getDepth() != 1 || images[3]->getDepth() != 6)
		{
			cerr << "Aborting denoising: expected depths 3 / 1 / 6 for color / number of samples / covariance images" << endl;
			return false;
		}
		return true;
	}

	bool Denoiser::layersAreOk()
	{
		if(m_layers.empty())
			return true;
		if(m_layers.size() > size_t(BCD_HIP_MAX_LAYERS - 1))
		{
			cerr << "Aborting denoising: " << m_layers.size() << " added colour layers, at most " << (BCD_HIP_MAX_LAYERS - 1) << " are supported" << endl;
			return false;
		}
		if(m_devices.size() > 1)
		{
			cerr << "Aborting denoising: colour layers are not available over several devices (row bands take one layer per call)" << endl;
			return false;
		}
		if(m_prefilterThresholdStDevFactor > 0.f && !m_prefilterLayers && !(m_prefilterFrames && !m_neighbourFrames.empty())) // (beside neighbour frames setSpikePrefilterFrames covers every layer)
		{
			cerr << "Aborting denoising: the spike prefilter moves whole pixels by the primary colours and is not available with added colour layers (setSpikePrefilterLayers(true) gathers every layer through its decision)" << endl;
			return false;
		}
		const int w = m_inputs.m_pColors->getWidth(), h = m_inputs.m_pColors->getHeight();
		for(size_t k = 0; k < m_layers.size(); ++k)
		{
			const ColorLayer& rLayer = m_layers[k];
			if(!rLayer.m_pColors || !rLayer.m_pSampleCovariances || !rLayer.m_pDenoisedColors)
			{
				cerr << "Aborting denoising: nullptr for an image of added colour layer " << k + 1 << endl;
				return false;
			}
			if(rLayer.m_pColors->getWidth() != w || rLayer.m_pColors->getHeight() != h || rLayer.m_pColors->getDepth() != 3 ||
					rLayer.m_pSampleCovariances->getWidth() != w || rLayer.m_pSampleCovariances->getHeight() != h || rLayer.m_pSampleCovariances->getDepth() != 6)
			{
				cerr << "Aborting denoising: added colour layer " << k + 1 << " must bring a " << w << "x" << h << "x3 color image and a "
						<< w << "x" << h << "x6 covariance image like the primary inputs" << endl;
				return false;
			}
			if(rLayer.m_pDenoisedColors == m_outputs.m_pDenoisedColors)
			{
				cerr << "Aborting denoising: added colour layer " << k + 1 << " writes into the primary output image" << endl;
				return false;
			}
			for(size_t j = 0; j < k; ++j)
				if(m_layers[j].m_pDenoisedColors == rLayer.m_pDenoisedColors)
				{
					cerr << "Aborting denoising: added colour layers " << j + 1 << " and " << k + 1 << " share an output image" << endl;
					return false;
				}
		}
		return true;
	}

	bool Denoiser::guideIsOk()
	{
		if(!m_pGuideFeatures)
			return true;
		if(m_devices.size() > 1)
		{
			cerr << "Aborting denoising: feature buffers (setGuideFeatures) are not available over several devices" << endl;
			return false;
		}
		const int w = m_inputs.m_pColors->getWidth(), h = m_inputs.m_pColors->getHeight();
		const int depth = m_pGuideFeatures->getDepth();
		if(m_pGuideFeatures->getWidth() != w || m_pGuideFeatures->getHeight() != h || depth < 1 || depth > BCD_HIP_GUIDE_MAX_CHANNELS)
		{
			cerr << "Aborting denoising: the feature image must be " << w << "x" << h << " like the input color image, with 1 to " << BCD_HIP_GUIDE_MAX_CHANNELS
					<< " channels (it is " << m_pGuideFeatures->getWidth() << "x" << m_pGuideFeatures->getHeight() << "x" << depth << ")" << endl;
			return false;
		}
		if(m_pGuideVariances && (m_pGuideVariances->getWidth() != w || m_pGuideVariances->getHeight() != h || m_pGuideVariances->getDepth() != depth))
		{
			cerr << "Aborting denoising: the feature variance image must be " << w << "x" << h << "x" << depth << " like the feature image" << endl;
			return false;
		}
		if(int(m_guideFloors.size()) != depth)
		{
			cerr << "Aborting denoising: " << m_guideFloors.size() << " feature floors for " << depth << " feature channels" << endl;
			return false;
		}
		// beside neighbour frames every neighbour brings its own feature buffers (setNeighbourGuideFeatures), shaped like the frame's
		for(size_t k = 0; k < m_neighbourFrames.size(); ++k)
		{
			const NeighbourGuide guide = k < m_neighbourGuides.size() ? m_neighbourGuides[k] : NeighbourGuide();
			if(!guide.m_pFeatures)
			{
				cerr << "Aborting denoising: neighbour frame " << k + 1 << " has no feature buffers (setNeighbourGuideFeatures) while the frame has (setGuideFeatures)" << endl;
				return false;
			}
			if(guide.m_pFeatures->getWidth() != w || guide.m_pFeatures->getHeight() != h || guide.m_pFeatures->getDepth() != depth)
			{
				cerr << "Aborting denoising: the feature image of neighbour frame " << k + 1 << " must be " << w << "x" << h << "x" << depth << " like the frame's feature image (it is "
						<< guide.m_pFeatures->getWidth() << "x" << guide.m_pFeatures->getHeight() << "x" << guide.m_pFeatures->getDepth() << ")" << endl;
				return false;
			}
			if((guide.m_pVariances != nullptr) != (m_pGuideVariances != nullptr))
			{
				cerr << "Aborting denoising: feature variances must be given for the frame and every neighbour frame or for none (neighbour frame " << k + 1 << " differs)" << endl;
				return false;
			}
			if(guide.m_pVariances && (guide.m_pVariances->getWidth() != w || guide.m_pVariances->getHeight() != h || guide.m_pVariances->getDepth() != depth))
			{
				cerr << "Aborting denoising: the feature variance image of neighbour frame " << k + 1 << " must be " << w << "x" << h << "x" << depth << " like the feature image" << endl;
				return false;
			}
		}
		return true;
	}

	namespace
	{
		/// Engine handles are kept for the life of the process, one per device (and one per device list): workspace, pyramid
		/// and staging buffers of the engine are grow-only, so a sequence of frames pays for them once.  A mutex per handle
		/// serialises callers (the reference's denoise() is not re-entrant either, src/core/Denoiser.cpp:114).
		struct EngineSlot
		{
			std::mutex m_mutex;
			bcd_hip_ctx* m_pCtx = nullptr;
			bcd_hip_multi* m_pMulti = nullptr;
			void release()
			{
				if(m_pCtx) bcd_hip_ctx_destroy(m_pCtx);
				if(m_pMulti) bcd_hip_multi_destroy(m_pMulti);
				m_pCtx = nullptr;
				m_pMulti = nullptr;
			}
		};
		std::mutex g_registryMutex;
		std::map< std::vector<int>, std::unique_ptr<EngineSlot> > g_registry;

		EngineSlot& engineSlot(const std::vector<int>& i_rDevices)
		{
			std::lock_guard<std::mutex> lock(g_registryMutex);
			std::unique_ptr<EngineSlot>& rSlot = g_registry[i_rDevices];
			if(!rSlot)
				rSlot.reset(new EngineSlot());
			return *rSlot;
		}

		// (the registry is deliberately not torn down by a static destructor: at process exit the HIP runtime may already be gone;
		//  bcd::releaseEngines() is the orderly way to give the memory back)

		void forwardProgress(float i_progress, void* i_pUser)
		{
			(*static_cast< std::function<void(float)>* >(i_pUser))(i_progress);
		}
	}

	void releaseEngines()
	{
		std::lock_guard<std::mutex> lock(g_registryMutex);
		for(auto& rEntry : g_registry)
		{
			std::lock_guard<std::mutex> slotLock(rEntry.second->m_mutex); // waits for a denoise() in flight on that slot
			rEntry.second->release();
		}
	}

	bool Denoiser::denoiseWithNbOfScales(int i_nbOfScales)
	{
		if(m_momentSelection && m_devices.size() > 1)
		{
			cerr << "Aborting denoising: the selection from means and covariances (setMomentSelection) is not available over several devices" << endl;
			return false;
		}
		if(!m_neighbourFrames.empty() && m_devices.size() > 1)
		{
			cerr << "Aborting denoising: neighbour frames (addNeighbourFrame) are not available over several devices" << endl;
			return false;
		}
		// neighbour frames under the moment selection (bcd_hip_denoise_temporal_moments_host): every neighbour must have been added by addNeighbourFrameMoments
		size_t nbOfMomentNeighbours = 0;
		for(size_t k = 0; k < m_neighbourFrames.size(); ++k)
			nbOfMomentNeighbours += (k < m_neighbourMoments.size() && m_neighbourMoments[k]) ? 1 : 0;
		if(nbOfMomentNeighbours > 0 && !m_momentSelection)
		{
			cerr << "Aborting denoising: neighbour frames added by addNeighbourFrameMoments need the selection from means and covariances (setMomentSelection(true))" << endl;
			return false;
		}
		if(!m_neighbourFrames.empty() && m_momentSelection && nbOfMomentNeighbours != m_neighbourFrames.size())
		{
			cerr << "Aborting denoising: neighbour frames (addNeighbourFrame) are not available with the moment selection: the cross-frame selection from means and covariances takes "
					"neighbours added by addNeighbourFrameMoments, and every neighbour must be added that way" << endl;
			return false;
		}
		const bool momentNeighbours = m_momentSelection && !m_neighbourFrames.empty();
		// setSpikePrefilterFrames(true): every frame of a call with neighbour frames passes through the prefilter (bcd_hip_denoise_temporal_host_ex)
		const bool prefilterFrames = m_prefilterFrames && m_prefilterThresholdStDevFactor > 0.f && !m_neighbourFrames.empty();
		if(!inputsOutputsAreOk() || !layersAreOk() || !guideIsOk())
			return false;
		m_width = m_inputs.m_pColors->getWidth();
		m_height = m_inputs.m_pColors->getHeight();
		m_nbOfPixels = m_width * m_height;
		if(prefilterFrames && (m_width < 3 || m_height < 3 || !std::isfinite(m_prefilterThresholdStDevFactor)))
		{
			cerr << "Aborting denoising: the spike prefilter of every frame (setSpikePrefilterFrames) needs a finite factor and frames of at least 3x3 pixels" << endl;
			return false;
		}
		if(momentNeighbours)
		{	// the size checks of the moment neighbours, before any device is asked for
			auto fits = [&](const DeepImage<float>* i_pImage, int i_depth)
			{
				return i_pImage && i_pImage->getWidth() == m_width && i_pImage->getHeight() == m_height && i_pImage->getDepth() == i_depth;
			};
			const size_t nbOfLayers = m_layers.size();
			bool ok = (!(m_prefilterThresholdStDevFactor > 0.f) || m_prefilterFrames) && m_neighbourLayers.size() == m_neighbourFrames.size() && m_neighbourMotion.size() == m_neighbourFrames.size();
			for(size_t k = 0; ok && k < m_neighbourFrames.size(); ++k)
			{
				const DenoiserInputs& f = m_neighbourFrames[k];
				ok = fits(f.m_pColors, 3) && fits(f.m_pNbOfSamples, 1) && fits(f.m_pSampleCovariances, 6) && m_neighbourLayers[k].size() == nbOfLayers;
				for(size_t j = 0; ok && j < nbOfLayers; ++j)
					ok = fits(m_neighbourLayers[k][j].m_pColors, 3) && fits(m_neighbourLayers[k][j].m_pSampleCovariances, 6);
				ok = ok && (!m_neighbourMotion[k] || fits(m_neighbourMotion[k], 2));
			}
			if(!ok)
			{
				cerr << "Aborting denoising: a neighbour frame of the moment selection (addNeighbourFrameMoments) needs colours, sample counts and covariances in the frame's size "
						"and, beside added layers, exactly one layer (addNeighbourFrameLayer) per added layer in that size, a motion field (setNeighbourMotion) has 2 channels in "
						"that size; neighbour frames do not combine with the spike prefilter" << endl;
				return false;
			}
		}
		// src/core/Denoiser.cpp:99-110,241-265: m_useCuda is a REQUEST in the reference -- "true" is declined with a note when the GPU path cannot serve
		// the call (no device, patch radius != 1) and the other path runs.  This library has one path, the HIP device, so it declines the opposite
		// request the same way: m_useCuda = false (--use-cuda 0) is answered with a note on cout and the device result, which is the CPU path's
		// within the 1e-4 the tests hold it to (round 5; scripts that pass --use-cuda 0 keep working).  A caller that must not get a device result
		// sets BCD_STRICT_CPU_REQUEST=1 in the environment: the request is then refused -- `false` and a message on cerr, before any device work.
		if(!m_parameters.m_useCuda)
		{
			const char* pStrict = getenv("BCD_STRICT_CPU_REQUEST");
			if(pStrict != nullptr && pStrict[0] == '1')
			{
				cerr << "Aborting denoising: m_useCuda = false (--use-cuda 0) requests the CPU/OpenMP path, which this build does not have, and "
						"BCD_STRICT_CPU_REQUEST=1 forbids answering it with the HIP device" << endl;
				return false;
			}
			cout << "Note: m_useCuda = false (--use-cuda 0) requests the CPU/OpenMP path, which this build does not have: running on the HIP device "
					"(set BCD_STRICT_CPU_REQUEST=1 to have such a request refused instead)" << endl;
		}
		// Denoiser.cpp:113-121: m_nbOfCores <= 0 means "OpenMP's default", and the ACTUAL thread count is written back -- the same number that
		// then decides the -r 0 visiting order (:375-380).  The loop runs on the device; the field keeps exactly that meaning here: the thread
		// count the reference would have run with.  Written back, it reproduces itself on the next denoise() of a reused object (a value
		// derived from scales x devices did not: frame 2 of a reused MultiscaleDenoiser visited in another order than frame 1)
		const int effectiveNbOfCores = m_parameters.m_nbOfCores > 0 ? m_parameters.m_nbOfCores : std::max(1, omp_get_max_threads());
		m_parameters.m_nbOfCores = effectiveNbOfCores;
		bcd_hip_params prm;
		bcd_hip_default_params(&prm);
		prm.hist_dist_threshold = m_parameters.m_histogramDistanceThreshold;
		prm.patch_radius = m_parameters.m_patchRadius;
		prm.search_radius = m_parameters.m_searchWindowRadius;
		prm.min_eigen_value = m_parameters.m_minEigenValue;
		// Denoiser.cpp:375-380: a shuffle (-r 1), else -- more than one thread -- the strip list (reorderPixelSetJumpNextStrip), else scanline.
		// The marking follows that list exactly (the reference's threads race through it).  The strip key packs the frame geometry into 32 bits
		// (bcd_common.h) and row bands over several devices mark in scanline order: outside those limits -r 0 falls back to the scanline
		// order -- the reference's own one-thread order -- with a note
		prm.use_random_pixel_order = m_parameters.m_useRandomPixelOrder ? 1 : 0;
		if(!m_parameters.m_useRandomPixelOrder && effectiveNbOfCores > 1)
		{
			const bool fits = m_width <= 8191 && m_height <= 8191 && m_parameters.m_patchRadius <= 3 && m_parameters.m_searchWindowRadius >= 1;
			if(m_devices.size() == 1 && fits)
				prm.use_random_pixel_order = 2;
			else
				cout << "Note: -r 0 with " << effectiveNbOfCores << " cores asks for the strip visiting order, which is not available "
						<< (fits ? "on several devices" : "for this frame geometry") << ": visiting in scanline order (the reference's one-core order)" << endl;
		}
		prm.marked_skip_probability = m_parameters.m_markedPixelsSkippingProbability;
		prm.order_seed = m_orderSeed;

		EngineSlot& rSlot = engineSlot(m_devices);
		std::lock_guard<std::mutex> lock(rSlot.m_mutex);
		m_progressCallback(0.f);
		Deepimf result(m_width, m_height, 3); // inputs may alias the output image (the CLI pre-copies colours into it)
		std::vector<Deepimf> layerResults(m_layers.size());
		const float* pIn[4] = { m_inputs.m_pColors->getDataPtr(), m_inputs.m_pNbOfSamples->getDataPtr(),
				m_momentSelection ? nullptr : m_inputs.m_pHistograms->getDataPtr(), m_inputs.m_pSampleCovariances->getDataPtr() };
		const int depth = m_momentSelection ? 0 : m_inputs.m_pHistograms->getDepth();
		int rc = BCD_HIP_OK;
		if(m_devices.size() > 1)
		{
			// the prefilter of the band path: SpikeRemovalFilter::filter on copies of the inputs (one device, whole frame: the filter is
			// 0.1 % of the work), like bcd_cli -p 1 does before denoise() (src/cli/main.cpp:428-441); the caller's images stay untouched
			Deepimf filtered[4];
			if(m_prefilterThresholdStDevFactor > 0.f)
			{
				filtered[0] = *m_inputs.m_pColors; filtered[1] = *m_inputs.m_pNbOfSamples;
				filtered[2] = *m_inputs.m_pHistograms; filtered[3] = *m_inputs.m_pSampleCovariances;
				if(!SpikeRemovalFilter::filterOnDevice(m_devices[0], filtered[0], filtered[1], filtered[2], filtered[3], m_prefilterThresholdStDevFactor))
				{
					cerr << "Aborting denoising: the spike prefilter failed on HIP device " << m_devices[0] << endl;
					return false;
				}
				for(int i = 0; i < 4; ++i)
					pIn[i] = filtered[i].getDataPtr();
			}
			if(!rSlot.m_pMulti && bcd_hip_multi_create(&rSlot.m_pMulti, m_devices.data(), int(m_devices.size())) != BCD_HIP_OK)
			{
				cerr << "Aborting denoising: unusable HIP device list (this build has no CPU path)" << endl;
				return false;
			}
			bcd_hip_multi_set_progress_callback(rSlot.m_pMulti, &forwardProgress, &m_progressCallback);
			rc = bcd_hip_multi_denoise_host(rSlot.m_pMulti, pIn[0], pIn[1], pIn[2], pIn[3], m_width, m_height, depth, i_nbOfScales, &prm, result.getDataPtr());
			bcd_hip_multi_set_progress_callback(rSlot.m_pMulti, nullptr, nullptr);
			if(rc != BCD_HIP_OK)
			{
				cerr << "Aborting denoising: " << bcd_hip_multi_last_error(rSlot.m_pMulti) << endl;
				// a failed frame may have left device work or communicators in an unknown state: the next call starts from a new handle
				bcd_hip_multi_destroy(rSlot.m_pMulti);
				rSlot.m_pMulti = nullptr;
			}
			else if(m_zeroBadOutputValues)
			{
				float* p = result.getDataPtr();
				for(size_t i = 0, n = size_t(m_nbOfPixels) * 3; i < n; ++i)
					if(!(p[i] >= 0.f) || !(p[i] <= std::numeric_limits<float>::max()))
						p[i] = 0.f;
			}
		}
		else
		{
			if(!rSlot.m_pCtx && bcd_hip_ctx_create(&rSlot.m_pCtx, m_devices[0], nullptr) != BCD_HIP_OK)
			{
				cerr << "Aborting denoising: no usable HIP device " << m_devices[0] << " (this build has no CPU path)" << endl;
				return false;
			}
			bcd_hip_set_progress_callback(rSlot.m_pCtx, &forwardProgress, &m_progressCallback);
			bcd_hip_host_options opt;
			opt.spike_factor = m_prefilterThresholdStDevFactor;
			opt.zero_bad_values = m_zeroBadOutputValues ? 1 : 0;
			if(momentNeighbours)
			{	// neighbour frames lend their means and covariances: no histogram anywhere; the primary images are layer 0 of every frame (sizes checked above)
				const size_t nbOfLayers = m_layers.size(), nbOfNeighbours = m_neighbourFrames.size();
				std::vector<bcd_hip_frame_layer> frameLayers(nbOfNeighbours * (nbOfLayers + 1));
				std::vector<bcd_hip_frame_layers> layeredFrames(nbOfNeighbours);
				std::vector<const float*> motion(nbOfNeighbours, nullptr);
				bool anyMotion = false;
				for(size_t k = 0; k < nbOfNeighbours; ++k)
				{
					const DenoiserInputs& f = m_neighbourFrames[k];
					bcd_hip_frame_layer* pLayers = &frameLayers[k * (nbOfLayers + 1)];
					pLayers[0] = { f.m_pColors->getDataPtr(), f.m_pSampleCovariances->getDataPtr() };
					for(size_t j = 0; j < nbOfLayers; ++j)
						pLayers[j + 1] = { m_neighbourLayers[k][j].m_pColors->getDataPtr(), m_neighbourLayers[k][j].m_pSampleCovariances->getDataPtr() };
					layeredFrames[k] = { f.m_pNbOfSamples->getDataPtr(), nullptr, pLayers, nullptr };
					if(m_neighbourMotion[k])
					{
						motion[k] = m_neighbourMotion[k]->getDataPtr();
						anyMotion = true;
					}
				}
				std::vector<bcd_hip_layer> layers(nbOfLayers + 1);
				layers[0] = { pIn[0], pIn[3], result.getDataPtr() };
				for(size_t k = 0; k < nbOfLayers; ++k)
				{
					layerResults[k].resize(m_width, m_height, 3);
					layers[k + 1] = { m_layers[k].m_pColors->getDataPtr(), m_layers[k].m_pSampleCovariances->getDataPtr(), layerResults[k].getDataPtr() };
				}
				bcd_hip_guide guide;
				std::vector<bcd_hip_guide_images> neighbourGuides(nbOfNeighbours);
				if(m_pGuideFeatures)
				{	// (guideIsOk has checked the neighbours' buffers)
					guide.features = m_pGuideFeatures->getDataPtr();
					guide.variances = m_pGuideVariances ? m_pGuideVariances->getDataPtr() : nullptr;
					guide.nb_channels = m_pGuideFeatures->getDepth();
					guide.floors = m_guideFloors.data();
					guide.threshold = m_guideThreshold;
					for(size_t k = 0; k < nbOfNeighbours; ++k)
						neighbourGuides[k] = { m_neighbourGuides[k].m_pFeatures->getDataPtr(), m_neighbourGuides[k].m_pVariances ? m_neighbourGuides[k].m_pVariances->getDataPtr() : nullptr };
				}
				if(prefilterFrames)
				{
					const bcd_hip_temporal_host_options frameOpt = { m_prefilterThresholdStDevFactor, nullptr };
					rc = bcd_hip_denoise_temporal_host_ex(rSlot.m_pCtx, pIn[1], nullptr, layeredFrames.data(), int(nbOfNeighbours), anyMotion ? motion.data() : nullptr, m_width,
							m_height, 0, i_nbOfScales, &prm, m_momentVarianceFloor, layers.data(), int(layers.size()), m_pGuideFeatures ? &guide : nullptr,
							m_pGuideFeatures ? neighbourGuides.data() : nullptr, &frameOpt);
				}
				else
				rc = bcd_hip_denoise_temporal_moments_host(rSlot.m_pCtx, pIn[1], layeredFrames.data(), int(nbOfNeighbours), anyMotion ? motion.data() : nullptr, m_width, m_height,
						i_nbOfScales, &prm, m_momentVarianceFloor, layers.data(), int(layers.size()), m_pGuideFeatures ? &guide : nullptr,
						m_pGuideFeatures ? neighbourGuides.data() : nullptr);
				if(rc == BCD_HIP_OK && m_zeroBadOutputValues)
				{
					for(size_t k = 0; k <= nbOfLayers; ++k)
					{
						float* p = k == 0 ? result.getDataPtr() : layerResults[k - 1].getDataPtr();
						for(size_t i = 0, n = size_t(m_nbOfPixels) * 3; i < n; ++i)
							if(!(p[i] >= 0.f) || !(p[i] <= std::numeric_limits<float>::max()))
								p[i] = 0.f;
					}
				}
			}
			else if(m_pGuideFeatures && m_neighbourFrames.empty())
			{	// the selection gated by the feature buffers: with histograms or, under setMomentSelection, without; the primary images are layer 0
				std::vector<bcd_hip_host_layer> layers(m_layers.size() + 1);
				layers[0].h_colors = pIn[0]; layers[0].h_covariances = pIn[3]; layers[0].h_out = result.getDataPtr();
				for(size_t k = 0; k < m_layers.size(); ++k)
				{
					layerResults[k].resize(m_width, m_height, 3);
					layers[k + 1].h_colors = m_layers[k].m_pColors->getDataPtr();
					layers[k + 1].h_covariances = m_layers[k].m_pSampleCovariances->getDataPtr();
					layers[k + 1].h_out = layerResults[k].getDataPtr();
				}
				bcd_hip_layers_host_options layersOpt = { opt.spike_factor, opt.zero_bad_values, m_prefilterLayers ? 1 : 0 };
				bcd_hip_guide guide;
				guide.features = m_pGuideFeatures->getDataPtr();
				guide.variances = m_pGuideVariances ? m_pGuideVariances->getDataPtr() : nullptr;
				guide.nb_channels = m_pGuideFeatures->getDepth();
				guide.floors = m_guideFloors.data();
				guide.threshold = m_guideThreshold;
				rc = bcd_hip_denoise_guided_host(rSlot.m_pCtx, pIn[1], pIn[2], m_width, m_height, depth, i_nbOfScales, &prm, &layersOpt, m_momentVarianceFloor, layers.data(),
						int(layers.size()), &guide);
			}
			else if(m_momentSelection)
			{	// no histogram: the primary images are the guide and layer 0, added layers follow on its selection
				std::vector<bcd_hip_host_layer> layers(m_layers.size() + 1);
				layers[0].h_colors = pIn[0]; layers[0].h_covariances = pIn[3]; layers[0].h_out = result.getDataPtr();
				for(size_t k = 0; k < m_layers.size(); ++k)
				{
					layerResults[k].resize(m_width, m_height, 3);
					layers[k + 1].h_colors = m_layers[k].m_pColors->getDataPtr();
					layers[k + 1].h_covariances = m_layers[k].m_pSampleCovariances->getDataPtr();
					layers[k + 1].h_out = layerResults[k].getDataPtr();
				}
				bcd_hip_layers_host_options layersOpt = { opt.spike_factor, opt.zero_bad_values, m_prefilterLayers ? 1 : 0 };
				rc = bcd_hip_denoise_moments_host(rSlot.m_pCtx, pIn[1], m_width, m_height, i_nbOfScales, &prm, &layersOpt, m_momentVarianceFloor, layers.data(), int(layers.size()));
			}
			else if(!m_neighbourFrames.empty())
			{	// neighbouring frames of the sequence lend their statistics; checked here: sizes, and what the call does not combine with
				std::vector<bcd_hip_frame> frames(m_neighbourFrames.size());
				const size_t nbOfLayers = m_layers.size();
				std::vector<bcd_hip_frame_layer> frameLayers(m_neighbourFrames.size() * (nbOfLayers + 1));
				std::vector<bcd_hip_frame_layers> layeredFrames(m_neighbourFrames.size());
				auto fits = [&](const DeepImage<float>* i_pImage, int i_depth)
				{
					return i_pImage && i_pImage->getWidth() == m_width && i_pImage->getHeight() == m_height && i_pImage->getDepth() == i_depth;
				};
				bool ok = (!(m_prefilterThresholdStDevFactor > 0.f) || m_prefilterFrames) && m_neighbourLayers.size() == m_neighbourFrames.size() && m_neighbourMotion.size() == m_neighbourFrames.size();
				std::vector<const float*> motion(m_neighbourFrames.size(), nullptr); // (a neighbour without a field: zero motion)
				bool anyMotion = false;
				for(size_t k = 0; ok && k < m_neighbourFrames.size(); ++k)
				{
					const DenoiserInputs& f = m_neighbourFrames[k];
					ok = fits(f.m_pColors, 3) && fits(f.m_pNbOfSamples, 1) && fits(f.m_pHistograms, depth) && fits(f.m_pSampleCovariances, 6)
							&& m_neighbourLayers[k].size() == nbOfLayers; // one layer of the neighbour per added layer of the frame
					for(size_t j = 0; ok && j < nbOfLayers; ++j)
						ok = fits(m_neighbourLayers[k][j].m_pColors, 3) && fits(m_neighbourLayers[k][j].m_pSampleCovariances, 6);
					ok = ok && (!m_neighbourMotion[k] || fits(m_neighbourMotion[k], 2));
					if(!ok)
						break;
					if(m_neighbourMotion[k])
					{
						motion[k] = m_neighbourMotion[k]->getDataPtr();
						anyMotion = true;
					}
					frames[k] = { f.m_pColors->getDataPtr(), f.m_pNbOfSamples->getDataPtr(), f.m_pHistograms->getDataPtr(), f.m_pSampleCovariances->getDataPtr(), nullptr };
					bcd_hip_frame_layer* pLayers = &frameLayers[k * (nbOfLayers + 1)];
					pLayers[0] = { f.m_pColors->getDataPtr(), f.m_pSampleCovariances->getDataPtr() }; // the primary images are layer 0
					for(size_t j = 0; j < nbOfLayers; ++j)
						pLayers[j + 1] = { m_neighbourLayers[k][j].m_pColors->getDataPtr(), m_neighbourLayers[k][j].m_pSampleCovariances->getDataPtr() };
					layeredFrames[k] = { f.m_pNbOfSamples->getDataPtr(), f.m_pHistograms->getDataPtr(), pLayers, nullptr };
				}
				if(!ok)
				{
					cerr << "Aborting denoising: a neighbour frame needs all four images in the frame's size and, beside added layers, exactly one layer "
							"(addNeighbourFrameLayer) per added layer in that size, a motion field (setNeighbourMotion) has 2 channels in that size; neighbour frames do "
							"not combine with the spike prefilter" << endl;
					bcd_hip_set_progress_callback(rSlot.m_pCtx, nullptr, nullptr);
					return false;
				}
				if(prefilterFrames)
				{	// every frame through the spike prefilter on its own, then the call its arguments name: layers, motion fields and the feature gate as without it
					std::vector<bcd_hip_layer> layers(nbOfLayers + 1);
					layers[0] = { pIn[0], pIn[3], result.getDataPtr() };
					for(size_t k = 0; k < nbOfLayers; ++k)
					{
						layerResults[k].resize(m_width, m_height, 3);
						layers[k + 1] = { m_layers[k].m_pColors->getDataPtr(), m_layers[k].m_pSampleCovariances->getDataPtr(), layerResults[k].getDataPtr() };
					}
					bcd_hip_guide guide;
					std::vector<bcd_hip_guide_images> neighbourGuides(m_neighbourFrames.size());
					if(m_pGuideFeatures)
					{	// (guideIsOk has checked the neighbours' buffers)
						guide.features = m_pGuideFeatures->getDataPtr();
						guide.variances = m_pGuideVariances ? m_pGuideVariances->getDataPtr() : nullptr;
						guide.nb_channels = m_pGuideFeatures->getDepth();
						guide.floors = m_guideFloors.data();
						guide.threshold = m_guideThreshold;
						for(size_t k = 0; k < m_neighbourFrames.size(); ++k)
							neighbourGuides[k] = { m_neighbourGuides[k].m_pFeatures->getDataPtr(), m_neighbourGuides[k].m_pVariances ? m_neighbourGuides[k].m_pVariances->getDataPtr() : nullptr };
					}
					const bcd_hip_temporal_host_options frameOpt = { m_prefilterThresholdStDevFactor, nullptr };
					rc = bcd_hip_denoise_temporal_host_ex(rSlot.m_pCtx, pIn[1], pIn[2], layeredFrames.data(), int(layeredFrames.size()), anyMotion ? motion.data() : nullptr, m_width,
							m_height, depth, i_nbOfScales, &prm, 0.f, layers.data(), int(layers.size()), m_pGuideFeatures ? &guide : nullptr,
							m_pGuideFeatures ? neighbourGuides.data() : nullptr, &frameOpt);
					if(rc == BCD_HIP_OK && m_zeroBadOutputValues)
						for(size_t k = 0; k < nbOfLayers; ++k)
						{
							float* p = layerResults[k].getDataPtr();
							for(size_t i = 0, n = size_t(m_nbOfPixels) * 3; i < n; ++i)
								if(!(p[i] >= 0.f) || !(p[i] <= std::numeric_limits<float>::max()))
									p[i] = 0.f;
						}
				}
				else if(m_pGuideFeatures)
				{	// the gate of the feature buffers on the in-frame and on every cross-frame selection (guideIsOk has checked the neighbours' buffers); the
					// primary images are layer 0 of every frame, added layers and motion fields as without the guide
					std::vector<bcd_hip_layer> layers(nbOfLayers + 1);
					layers[0] = { pIn[0], pIn[3], result.getDataPtr() };
					for(size_t k = 0; k < nbOfLayers; ++k)
					{
						layerResults[k].resize(m_width, m_height, 3);
						layers[k + 1] = { m_layers[k].m_pColors->getDataPtr(), m_layers[k].m_pSampleCovariances->getDataPtr(), layerResults[k].getDataPtr() };
					}
					bcd_hip_guide guide;
					guide.features = m_pGuideFeatures->getDataPtr();
					guide.variances = m_pGuideVariances ? m_pGuideVariances->getDataPtr() : nullptr;
					guide.nb_channels = m_pGuideFeatures->getDepth();
					guide.floors = m_guideFloors.data();
					guide.threshold = m_guideThreshold;
					std::vector<bcd_hip_guide_images> neighbourGuides(m_neighbourFrames.size());
					for(size_t k = 0; k < m_neighbourFrames.size(); ++k)
						neighbourGuides[k] = { m_neighbourGuides[k].m_pFeatures->getDataPtr(), m_neighbourGuides[k].m_pVariances ? m_neighbourGuides[k].m_pVariances->getDataPtr() : nullptr };
					rc = bcd_hip_denoise_temporal_guided_host(rSlot.m_pCtx, pIn[1], pIn[2], layeredFrames.data(), int(layeredFrames.size()), anyMotion ? motion.data() : nullptr, m_width,
							m_height, depth, i_nbOfScales, &prm, layers.data(), int(layers.size()), &guide, neighbourGuides.data());
					if(rc == BCD_HIP_OK && m_zeroBadOutputValues)
						for(size_t k = 0; k < nbOfLayers; ++k)
						{
							float* p = layerResults[k].getDataPtr();
							for(size_t i = 0, n = size_t(m_nbOfPixels) * 3; i < n; ++i)
								if(!(p[i] >= 0.f) || !(p[i] <= std::numeric_limits<float>::max()))
									p[i] = 0.f;
						}
				}
				else if(nbOfLayers == 0 && anyMotion)
					rc = bcd_hip_denoise_temporal_motion_host(rSlot.m_pCtx, pIn[0], pIn[1], pIn[2], pIn[3], frames.data(), int(frames.size()), motion.data(), m_width, m_height, depth,
							i_nbOfScales, &prm, result.getDataPtr());
				else if(nbOfLayers == 0)
					rc = bcd_hip_denoise_temporal_host(rSlot.m_pCtx, pIn[0], pIn[1], pIn[2], pIn[3], frames.data(), int(frames.size()), m_width, m_height, depth, i_nbOfScales, &prm,
							result.getDataPtr());
				else
				{	// the primary images are layer 0 of every frame: one selection over all frames serves every layer
					std::vector<bcd_hip_layer> layers(nbOfLayers + 1);
					layers[0] = { pIn[0], pIn[3], result.getDataPtr() };
					for(size_t k = 0; k < nbOfLayers; ++k)
					{
						layerResults[k].resize(m_width, m_height, 3);
						layers[k + 1] = { m_layers[k].m_pColors->getDataPtr(), m_layers[k].m_pSampleCovariances->getDataPtr(), layerResults[k].getDataPtr() };
					}
					if(anyMotion)
						rc = bcd_hip_denoise_temporal_layers_motion_host(rSlot.m_pCtx, pIn[1], pIn[2], layeredFrames.data(), int(layeredFrames.size()), motion.data(), m_width, m_height,
								depth, i_nbOfScales, &prm, layers.data(), int(layers.size()));
					else
						rc = bcd_hip_denoise_temporal_layers_host(rSlot.m_pCtx, pIn[1], pIn[2], layeredFrames.data(), int(layeredFrames.size()), m_width, m_height, depth, i_nbOfScales,
								&prm, layers.data(), int(layers.size()));
					if(rc == BCD_HIP_OK && m_zeroBadOutputValues)
						for(size_t k = 0; k < nbOfLayers; ++k)
						{
							float* p = layerResults[k].getDataPtr();
							for(size_t i = 0, n = size_t(m_nbOfPixels) * 3; i < n; ++i)
								if(!(p[i] >= 0.f) || !(p[i] <= std::numeric_limits<float>::max()))
									p[i] = 0.f;
						}
				}
				if(rc == BCD_HIP_OK && m_zeroBadOutputValues)
				{
					float* p = result.getDataPtr();
					for(size_t i = 0, n = size_t(m_nbOfPixels) * 3; i < n; ++i)
						if(!(p[i] >= 0.f) || !(p[i] <= std::numeric_limits<float>::max()))
							p[i] = 0.f;
				}
			}
			else if(m_layers.empty())
				rc = bcd_hip_denoise_host_ex(rSlot.m_pCtx, pIn[0], pIn[1], pIn[2], pIn[3], m_width, m_height, depth, i_nbOfScales, &prm, &opt, result.getDataPtr());
			else
			{	// the primary images are layer 0: one selection of similar patches serves every layer
				std::vector<bcd_hip_host_layer> layers(m_layers.size() + 1);
				layers[0].h_colors = pIn[0]; layers[0].h_covariances = pIn[3]; layers[0].h_out = result.getDataPtr();
				for(size_t k = 0; k < m_layers.size(); ++k)
				{
					layerResults[k].resize(m_width, m_height, 3);
					layers[k + 1].h_colors = m_layers[k].m_pColors->getDataPtr();
					layers[k + 1].h_covariances = m_layers[k].m_pSampleCovariances->getDataPtr();
					layers[k + 1].h_out = layerResults[k].getDataPtr();
				}
				if(m_prefilterLayers)
				{	// the prefilter covers every layer: gathered on the device through the source map of the primary colours
					bcd_hip_layers_host_options layersOpt = { opt.spike_factor, opt.zero_bad_values, 1 };
					rc = bcd_hip_denoise_layers_host_ex(rSlot.m_pCtx, pIn[1], pIn[2], m_width, m_height, depth, i_nbOfScales, &prm, &layersOpt, layers.data(), int(layers.size()));
				}
				else
					rc = bcd_hip_denoise_layers_host(rSlot.m_pCtx, pIn[1], pIn[2], m_width, m_height, depth, i_nbOfScales, &prm, &opt, layers.data(), int(layers.size()));
			}
			bcd_hip_set_progress_callback(rSlot.m_pCtx, nullptr, nullptr);
			if(rc != BCD_HIP_OK)
			{
				cerr << "Aborting denoising: " << bcd_hip_last_error(rSlot.m_pCtx) << endl;
				if(rc == BCD_HIP_EDEVICE || rc == BCD_HIP_ENOMEM)
				{	// device error / out of memory: give everything back, the next call builds a new context
					bcd_hip_ctx_destroy(rSlot.m_pCtx);
					rSlot.m_pCtx = nullptr;
				}
			}
		}
		if(rc != BCD_HIP_OK)
			return false;
		*m_outputs.m_pDenoisedColors = std::move(result); // resized to W x H x 3 and overwritten (Denoiser.cpp:207-208)
		for(size_t k = 0; k < m_layers.size(); ++k)
			*m_layers[k].m_pDenoisedColors = std::move(layerResults[k]);
		m_progressCallback(1.f);
		return true;
	}

	bool Denoiser::denoise()
	{
		return denoiseWithNbOfScales(1);
	}

	bool MultiscaleDenoiser::denoise()
	{
		if(m_nbOfScales < 1)
		{
			cerr << "Aborting denoising: number of scales must be >= 1" << endl;
			return false;
		}
		// the pyramid (MultiscaleDenoiser.cpp:41-53), the per-scale denoisers (:79-134) and the merges (:453-466) are one engine
		// call; a Denoiser configured like this object makes it
		Denoiser engine;
		engine.setInputs(m_inputs);
		engine.setOutputs(m_outputs);
		engine.setParameters(m_parameters);
		engine.setProgressCallback(m_progressCallback);
		engine.setOrderSeed(m_orderSeed);
		engine.setDevices(m_devices);
		engine.setSpikePrefilter(m_prefilterThresholdStDevFactor);
		engine.setZeroBadOutputValues(m_zeroBadOutputValues);
		engine.setLayers(m_layers);
		engine.setNeighbourFrames(m_neighbourFrames);
		engine.setNeighbourFrameLayers(m_neighbourLayers);
		engine.setNeighbourMotions(m_neighbourMotion);
		engine.setNeighbourGuides(m_neighbourGuides);
		engine.setNeighbourMomentFlags(m_neighbourMoments);
		engine.setSpikePrefilterLayers(m_prefilterLayers);
		engine.setSpikePrefilterFrames(m_prefilterFrames);
		engine.setMomentSelection(m_momentSelection, m_momentVarianceFloor);
		engine.setGuideFeatures(m_pGuideFeatures, m_pGuideVariances, m_guideFloors, m_guideThreshold);
		const bool ok = engine.denoiseWithNbOfScales(m_nbOfScales);
		m_parameters.m_nbOfCores = engine.getParameters().m_nbOfCores;
		return ok;
	}

} // namespace bcd
