// SequenceDenoiser.h -- the frames of an animation denoised through a sliding window (MI355X build; bcd_hip_sequence_* of include/bcd_hip.h).
// Denoiser::addNeighbourFrame denoises one frame with its neighbours and forgets everything: called once per frame of an animation it uploads every frame,
// builds its pyramid and searches every pair of frames 2 R + 1 times.  A SequenceDenoiser takes the frames one by one, keeps the last 2 R + 1 on the
// device, and hands back frame t denoised with the frames t - R .. t + R that exist -- what a Denoiser / MultiscaleDenoiser with those neighbours added in
// ascending order returns for it -- with every frame uploaded once and every pair of frames searched once.
#ifndef SEQUENCE_DENOISER_H
#define SEQUENCE_DENOISER_H

#include "Denoiser.h"

#include <cstdint>
#include <string>

namespace bcd
{

	/// Usage: setParameters / setOrderSeed / setDevice as on a Denoiser, then per frame pushFrame(), and popFrame() while ready() > 0; after the last frame
	/// end(), and popFrame() until ready() is 0.  Frame t can be popped once frame t + R is pushed, or after end(); a push is refused while the window is
	/// full (pop first).  The settings of HipEngineSettings that a sequence does not serve -- added layers, neighbour frames of its own, the moment
	/// selection, feature buffers, the spike prefilter, several devices -- make pushFrame() return false, like a patch radius other than 1, a search
	/// radius other than 6 or a temporal radius outside 1 .. 2; every refusal comes before any device is asked for, with a message on cerr.
	class SequenceDenoiser : public HipEngineSettings
	{
	public:
		SequenceDenoiser(int i_nbOfScales = 1, int i_temporalRadius = 1);
		~SequenceDenoiser();
		SequenceDenoiser(const SequenceDenoiser&) = delete;
		SequenceDenoiser& operator=(const SequenceDenoiser&) = delete;

		const DenoiserParameters& getParameters() const { return m_parameters; }
		/// copied when the first frame is pushed; later changes take effect after reset()
		void setParameters(const DenoiserParameters& i_rParameters) { m_parameters = i_rParameters; }
		int getNbOfScales() const { return m_nbOfScales; }
		int getTemporalRadius() const { return m_temporalRadius; }

		/// the next frame: the four images are uploaded before the call returns.  The first frame fixes width, height and histogram depth
		bool pushFrame(const DenoiserInputs& i_rFrame);
		/// no further frame follows: the frames still held become ready
		bool end();
		/// frames that popFrame() can deliver now
		int ready() const;
		/// the next frame in push order; o_rOutputs.m_pDenoisedColors is resized to W x H x 3 and overwritten
		bool popFrame(DenoiserOutputs& o_rOutputs);
		/// index (from 0, in push order) of the frame the last successful popFrame() delivered, -1 before
		int64_t getLastFrameIndex() const { return m_lastFrameIndex; }
		/// forgets every frame (the device buffers stay) and takes the current parameters and settings for the next sequence
		void reset();

		/// the checks of pushFrame() that need no device, without the push (what bcd_cli runs on its arguments)
		bool settingsAreOk() const;

	private:
		bool frameIsOk(const DenoiserInputs& i_rFrame) const;
		void release();

		DenoiserParameters m_parameters;
		int m_nbOfScales;
		int m_temporalRadius;
		void* m_pCtx;      // bcd_hip_ctx of this object (created by the first push)
		void* m_pSequence; // bcd_hip_sequence_* handle
		int m_width, m_height, m_depth;
		int64_t m_lastFrameIndex;
	};

} // namespace bcd

#endif // SEQUENCE_DENOISER_H
