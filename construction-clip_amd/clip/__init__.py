"""Drop-in for `import clip` (openai/CLIP's public surface as used by zhuluntsai/Construction-CLIP),
executing on MI355X through libcclip_hip.so.  See clip.py / model.py."""
from .clip import available_models, load, tokenize, _transform  # noqa: F401
from . import simple_tokenizer  # noqa: F401  (attention.py:114 uses clip.simple_tokenizer.SimpleTokenizer)
from .model import CLIP, build_model  # noqa: F401
from .loss import contrastive_loss, ContrastiveLoss, class_ids, unique_texts  # noqa: F401
from .loss import sigmoid_loss, SigmoidLoss  # noqa: F401  (SigLIP's pairwise sigmoid objective on the same head)
from .loss import distill_loss, DistillLoss  # noqa: F401  (KL to a frozen teacher's similarity rows, same head)
from .preprocess_device import DevicePreprocess  # noqa: F401
from .explain import interpret, image_relevance_map, text_token_scores  # noqa: F401  (attention.py:14, 88-92, 115-117)
from .explain import interpret_rows, text_row_scores  # noqa: F401  (the same rows for towers of more than 128 tokens)
from .explain import jet_table, relevance_overlay, text_heat_html  # noqa: F401  (attention.py:77-96, 113-143: the overlay picture)
from .retrieval import EmbeddingIndex, retrieval_recall  # noqa: F401  (search over the embedding pickle; image <-> text R@k)
from .retrieval import connected_components, group_split  # noqa: F401  (near-duplicate groups and leak-free held-out splits)
from .hubness import fit_querybank, QueryBank, hubness, HubnessReport  # noqa: F401  (hubness-corrected retrieval: inverted softmax, QB-Norm, CSLS)
from .cluster import kmeans, KMeansResult, cluster_purity, name_clusters  # noqa: F401  (spherical k-means of the unlabelled photos)
from .tsne import tsne, TSNEResult  # noqa: F401  (a 2-D map of the stored embeddings on the kNN graph)
from .propagate import spread_labels, LabelSpreadResult, affinity_csr  # noqa: F401  (label spreading: a few labels over the kNN graph)
from .coreset import select_coreset, CoresetResult  # noqa: F401  (k-centre greedy selection: which photos to label next)
from .hdbscan import hdbscan, HDBSCANResult, mutual_reachability_mst, MSTResult  # noqa: F401  (density clusters without a k, on an exact spanning tree)
from .concepts import ConceptDictionary, ConceptDecomposition, ConceptProfile, decompose, concept_profile, distinctive  # noqa: F401  (sparse non-negative concept codes: what is in an embedding, in words)
from .fewshot import CacheClassifier, confusion_matrix  # noqa: F401  (few-shot classification from the stored, labelled embeddings)
from .probe import LinearProbe, ProbeLossFunction, ProbeFitResult  # noqa: F401  (linear probe: logistic regression on the stored embeddings)
from .gaussian import GaussianClassifier, ClassMoments, MahalanobisScores, PCAResult, class_moments, pca  # noqa: F401  (Gaussian class models: training-free classifier, outlier scores, PCA)
from .regions import encode_regions, classify_regions  # noqa: F401  (embed / zero-shot-classify every detector box of a photo)
from .dense import segment, dense_features, DenseResult, default_palette  # noqa: F401  (dense zero-shot maps: per-patch class probabilities, label maps)
from .dense import segment_photo, plan_windows, PhotoDenseResult, label_boxes  # noqa: F401  (whole photos: sliding windows stitched in one launch)
from .dense import label_components, ComponentsResult  # noqa: F401  (instances: connected components of a label map, on the device)
from .dense import refine_maps, RefinedDenseResult  # noqa: F401  (boundaries: image-guided refinement of the class maps, PAMR)
from .dense import evaluate_labels, SegmentationScores  # noqa: F401  (evaluation: mean IoU and boundary IoU against ground-truth masks)
from .dense_fewshot import DensePrototypes  # noqa: F401  (few-shot dense maps: class prototypes pooled under annotated masks)
from .score import ClipScores, clip_score, clip_score_features  # noqa: F401  (CLIPScore / RefCLIPScore, best-of-K caption selection)
