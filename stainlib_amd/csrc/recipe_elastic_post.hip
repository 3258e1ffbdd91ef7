// recipe_elastic_post.hip -- the one-pass recipe (recipe_kernels.hpp; launchers: recipe_launch.hpp): the elastic view with the post stage.
// One of the translation units the recipe's kernel families are spread over, so that a parallel build compiles them side by side.
#include "recipe_launch.hpp"

template int sl::recipe_launch_elastic<0, true>(const sl::RecipeCall&);
