"""`speecht-cli search` -- local (evolutionary) search over the three scorer weights of the LM-scored beam search
(speecht/parameter_search.py restated).

The reference's walk: the first candidate is (lm_weight, word_count_weight, valid_word_count_weight) = (1.0, 0.0, 0.0); every
further one is ``random.choice`` of the population mutated by three ``np.random.normal(0, noise_std)`` draws (lm, wc, valid wc, in
that order), scored on a batch of its own from the endlessly looping dev set, ``bisect.insort``-ed into the population, which
drops its lowest member once it holds more than ``population_size``; every new candidate is printed as it comes (``--ui``: the
curses population view instead).  The score is -(global LER + global WER) of the batch.

Scoring does not run the reference's ``run_step`` per candidate: one forward pass per batch, the candidates' searches in ONE
launch (engine.lm_beam_search_decode_candidates) and all their edit distances in one more (candidate_scoring.score_candidates),
with the statistics ``run_step`` would give.

Extensions: ``max_iterations`` (stop after that many new candidates and print the population best-first; 0 = run until
stopped), and ``candidates_per_batch`` = K > 1, which CHANGES THE WALK: a generation draws K parents from the population as it
stands (K ``random.choice`` calls, then the mutations of the children in order), scores the K children on one batch, then
inserts and prints them in the order they were drawn.  The last generation before ``max_iterations`` draws only as many as are
left.  K = 1 is the reference's walk."""
import bisect
import random

import numpy as np

from .evaluation import EvalStatistics, Evaluation


class Candidate:

  def __init__(self, lm_weight: float, word_count_weight: float, valid_word_count_weight: float):
    self.score = None
    self.stats = None
    self.lm_weight = lm_weight
    self.word_count_weight = word_count_weight
    self.valid_word_count_weight = valid_word_count_weight

  def __gt__(self, other):
    return self.score > other.score

  def __lt__(self, other):
    return self.score < other.score

  def __str__(self):
    return ('{:.2f} Candidate (lm_weight={:.2f}, wc_weight={:.2f}, valid_wc_weight={:.2f}) has LER: {:.2f} WER: {:.2f}'.format(
        self.score, self.lm_weight, self.word_count_weight, self.valid_word_count_weight, self.stats.global_letter_error_rate,
        self.stats.global_word_error_rate))

  @property
  def weights(self):
    return (self.lm_weight, self.word_count_weight, self.valid_word_count_weight)

  def update_score(self, score: float, stats: EvalStatistics):
    self.score = score
    self.stats = stats

  @staticmethod
  def random_noise(std: float):
    return np.random.normal(loc=0, scale=std)

  def mutate(self, std: float):
    # (keyword arguments are evaluated left to right: the draws go to lm, wc, valid wc in that order)
    return Candidate(lm_weight=self.lm_weight + self.random_noise(std),
                     word_count_weight=self.word_count_weight + self.random_noise(std),
                     valid_word_count_weight=self.valid_word_count_weight + self.random_noise(std))


class LanguageModelParameterSearch(Evaluation):

  def __init__(self, flags):
    super().__init__(flags)
    self.candidates = []
    self.num_iterations = 0

  def create_sample_generator(self, limit_count: int):
    return self.reader.load_samples('dev', loop_infinitely=True, limit_count=limit_count, feature_type=self.flags.feature_type,
                                    shuffle_seed=self.shuffle_seed)

  def get_loader_limit_count(self):
    return 0

  def get_max_steps(self):
    return None

  # -- scoring ---------------------------------------------------------------------------------
  def score_candidates(self, model, sess, candidates):
    """One batch: a forward pass, the candidates' LM searches in one launch, their statistics; sets every candidate's score."""
    from .candidate_scoring import score_candidates
    label, = model.step(sess, loss=False, update=False, decode=False, return_label=True)
    decodes = model.engine.lm_beam_search_decode_candidates(model.language_model, [c.weights for c in candidates],
                                                            model.beam_width, model.beam_input)
    every = score_candidates(label, decodes, pair_by_row=getattr(self.flags, 'pair_by_row', False),
                             device=not getattr(self.flags, 'host_scoring', False))
    for candidate, stats in zip(candidates, every):
      candidate.update_score(-(stats.global_letter_error_rate + stats.global_word_error_rate), stats)

  # -- the walk --------------------------------------------------------------------------------
  def search(self, score, should_stop=lambda: False, stdscr=None, max_iterations=0, candidates_per_batch=1):
    """The search loop; ``score(list of candidates)`` sets their scores (one batch per call)."""
    if stdscr:
      stdscr.clear()
      stdscr.addstr(0, 0, 'Loading...')
      stdscr.refresh()
    first = Candidate(1.0, 0.0, 0.0)
    score([first])
    self.candidates.append(first)
    self._show(stdscr, first)
    while not should_stop() and not (max_iterations and self.num_iterations >= max_iterations):
      k = candidates_per_batch
      if max_iterations:
        k = min(k, max_iterations - self.num_iterations)
      parents = [random.choice(self.candidates) for _ in range(k)]
      children = [parent.mutate(self.flags.noise_std) for parent in parents]
      score(children)
      for child in children:
        # Note: tiny populations, so O(n) insertion is not an issue
        bisect.insort(self.candidates, child)
        if len(self.candidates) > self.flags.population_size:
          del self.candidates[0]
        self.num_iterations += 1
        self._show(stdscr, child)

  def _show(self, stdscr, candidate):
    if stdscr:
      self.print_population(stdscr)
    else:
      print(candidate)

  def population_lines(self):
    return ['Current population after {} iterations'.format(self.num_iterations), ''] + [str(c) for c in reversed(self.candidates)]

  def print_population(self, stdscr):
    stdscr.clear()
    for idx, line in enumerate(self.population_lines()):
      if line:
        stdscr.addstr(idx, 0, line)
    stdscr.refresh()

  def run(self):
    from . import speech_model
    seed = getattr(self.flags, 'seed', None)
    if seed is not None:
      random.seed(seed)
      np.random.seed(seed)
    max_iterations = getattr(self.flags, 'max_iterations', 0) or 0
    per_batch = max(1, getattr(self.flags, 'candidates_per_batch', 1) or 1)
    with speech_model.Session(getattr(self.flags, 'device', 'cuda:0')) as sess:
      model = self.create_model(sess)
      coordinator = self.start_pipeline(sess)
      try:
        def run_search(stdscr=None):
          self.search(lambda cands: self.score_candidates(model, sess, cands), coordinator.should_stop, stdscr, max_iterations,
                      per_batch)
        if getattr(self.flags, 'use_ui', False):
          from curses import wrapper
          wrapper(run_search)
        else:
          run_search()
      finally:
        coordinator.request_stop()
        coordinator.join()
    if max_iterations:
      for line in self.population_lines():
        print(line)
    return self.candidates
